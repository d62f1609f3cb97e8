"""Command areas on the host (include/elmk.h "command areas", C0 - C8): the numpy restatement (routing.command_allot, command_take,
kinematic_call(dam={..., "command": cmd})) held against five wrong variants, the census of the device test's inputs, C5's closure in
exact rational arithmetic, a dam above a dry crop cell, the supply limit's C6, routing.check_command text by text, and elmk_maps.h's
command_check as a stand-alone program, plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import command_cases as cc
from tests import reservoir_cases as rc
from tests.support import ROOT, bits

U = 2.0 ** -53
N = 1001
DT, NSUB = 1800.0, 3
NAN, INF = float("nan"), float("inf")


def _inputs(area, call):
    """R1's aggregates with idle cells: every sixteenth cell (c % 16 == 4) withdraws nothing, every odd cell half its runoff."""
    rn, i = rc.aggregates(N, 5, call)
    c = np.arange(N)
    i = np.where(c % 16 == 4, 0.0, np.where(c % 2 == 0, i, 0.5 * rn))
    with np.errstate(all="ignore"):
        qin = ((rn - i) * 0.001) * area
    return qin, 0.3 * np.abs(qin), (rn, i)


@pytest.fixture(scope="module")
def forest():
    """The 1001-cell forest of the device test with its cells and dams, edge values taken out of the storages (the census and the
    closure are about finite water), and the dependency rows of command_cases.command_values."""
    ddist, area, p0, volr, wh, wt = rc.cell_values(N, 40 + N)
    rdepth, eprof, p, volr, wh, wt, wf = rc.flood_values(N, 60 + N, area, p0, volr, wh, wt, NSUB, DT)
    fin = lambda x: np.where(np.isfinite(x) & (np.abs(x) < 1e200) & (x >= 0.0), x, 7.0)  # noqa: E731
    volr, wh, wt = (fin(x) for x in (volr, wh, wt))
    area = np.where(area > 0.0, area, 1.0e8)
    cap, target, beta, mstart, res, krls = rc.dam_values(N, 90 + N)
    for lo, edges in ((rc.RES_EDGE0, rc.SPECIAL), (rc.CAP_EDGE0, rc.CAP_EDGES)):
        for i in range(len(edges)):
            cap[lo + 2 * i], res[lo + 2 * i] = 0.0, 0.0  # (the dams are reservoir_cases.dam_cells', and no other)
    cap[rc.dam_cells(N)] = np.maximum(cap[rc.dam_cells(N)], 1.0e8)
    res = fin(res)
    down = rc.networks(N, 52 + N)["forest"]
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    cmd = rt.command_tables(cap, *cc.command_values(N, 3, _inputs(area, 0)[2][1] > 0.0))
    return down, rt.upstream_map(down), area, p, (wh, wt, volr), tab, cmd, res, krls


def _call(forest, state, c, variant=None, census=None):
    down, up, area, p, _, tab, cmd, _, _ = forest
    wh, wt, volr, res, krls, rows = state
    month, begins = rc.call_time(c % 12)
    qin, qsur, wd = _inputs(area, c)
    command = dict(cmd, variant=variant, census=census, take=rows[1], give=rows[2], ratio=rows[3])
    dam = {"tab": tab, "res": res, "krls": krls, "month": month, "begins": begins, "withdrawal": wd, "command": command}
    return rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, DT, NSUB, dam=dam), (qin, qsur, wd)


def _start(forest):
    wh, wt, volr = forest[4]
    return wh, wt, volr, forest[7], forest[8], (None, None, None, None)


def _next(out):
    return out[0], out[1], out[2], out[4], out[5], out[-4:]


# ---- 1. the census ----------------------------------------------------------------------------------------------------------------------
def test_every_item_of_the_census_occurs_in_every_call(forest):
    """Five chained calls on the forest: limited dams, unlimited dams with W > 0, dams with terms and W = 0, dams without terms, dams at
    or below SMIN, cells of one, two and four slots, a cell on a limited and an unlimited dam at once, dam cells that depend on another
    dam and cells with rest <= 0 - each in every call; a ratio strictly between 0 and 1 in every call; TAKE only where a slot is
    filled, GIVE only at dams with terms."""
    tab, cmd = forest[5], forest[6]
    state = _start(forest)
    for c in range(rc.NCALLS):
        seen = {}
        out, _ = _call(forest, state, c, census=seen)
        want, take, give, ratio = out[-4:]
        held = cc.census(cmd, tab, want, seen, ratio)
        assert all(held[k] > 0 for k in cc.CENSUS), (c, held)
        assert ((ratio > 0.0) & (ratio < 1.0)).any() and (ratio[~tab["DAM"]] == 1.0).all()
        assert not take[~cmd["HAS"]].any() and not want[~cmd["HAS"]].any() and (take[cmd["HAS"]] > 0.0).any()
        with_terms = np.zeros(N, bool)
        with_terms[cmd["dams"][np.diff(cmd["ptr"]) > 0]] = True
        assert not give[~with_terms].any() and (give[with_terms] > 0.0).any()
        state = _next(out)
    nd = cmd["dams"].size
    assert nd == 143 and nd > 2 * cc.CMD_DAMS  # the dam list crosses two workgroups of k_command_allot


# ---- 2. C0 --------------------------------------------------------------------------------------------------------------------------------
def test_no_filled_slot_gives_the_bits_of_the_form_without_the_part(forest):
    """Rows without a filled slot: every row of kinematic_call(dam=) without "command", bit for bit; WANT, TAKE and GIVE zero, RATIO 1."""
    down, up, area, p, (wh, wt, volr), tab, _, res, krls = forest
    empty = rt.command_tables(tab["CAP"], np.full((4, N), -1), np.full((4, N), NAN), np.full((4, N), -3.0))
    assert not empty["HAS"].any() and empty["ptr"][-1] == 0 and empty["dams"].size == int(tab["DAM"].sum())
    qin, qsur, wd = _inputs(area, 0)
    dam = {"tab": tab, "res": res, "krls": krls, "month": 3, "begins": True, "withdrawal": wd}
    plain = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, DT, NSUB, dam=dam)
    got = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, DT, NSUB, dam=dict(dam, command=empty))
    for g, w in zip(got, plain):
        assert bits(g) == bits(w)
    want, take, give, ratio = got[-4:]
    assert not want.any() and not take.any() and not give.any() and bits(ratio) == bits(np.ones(N))
    # C8: a NaN rest (a NaN withdrawal) asks for nothing; an infinite one asks for +inf
    one = {"HAS": np.ones(3, bool)}
    assert rt.command_want(np.array([NAN, INF, -1.0]), DT, one).tolist() == [0.0, INF, 0.0]


# ---- 3. closure, and the wrong variants ---------------------------------------------------------------------------------------------------
def _fsum(x):
    """The exact sum of finite doubles (every one is a multiple of 2^-1074)."""
    total = 0
    for v in np.asarray(x, dtype=np.float64).tolist():
        n, d = v.as_integer_ratio()
        total += n * ((1 << 1074) // d)
    return Fraction(total, 1 << 1074)


def _closure(forest, ncall, variant=None):
    """ncall chained calls.  Returns (the largest |accumulated residual| of C5's closure, the sum of the calls' bounds, the largest
    |sum GIVE - sum TAKE| of a call over its bound, the lowest RES - min(SMIN, first RES) over the dams with terms).

    The residual of one call, in exact rational arithmetic on the doubles:
        sum(WH + WT + VOLR + RES)_end - sum(..)_beg - dt (sum QIN - sum outlet QOUT) + sum RES_TAKE + sum CMD_GIVE,
    with QIN the credited row.  test_routing_reservoir_host.py counts the roundings of a call with dams as
        1.01 u (17 nsub SC + 5 dt Q + (nsub + 1) nsub SC + dt (SQ + SO) + 8 nsub SC + SC),   SC = S at the call's start + dt Q.
    The part adds: RES - G, one rounding of magnitude at most RES per dam, at most u SC; got / dt and QIN + got / dt, which times dt are
    u TAKE and u dt |QIN| per cell, at most u (T + dt SQ) with T = sum TAKE; and the difference between what the dams gave and what the
    cells received.  GIVE = fl(W ratio) with W the rounded sum of a dam's nt products x: |W - sum x| <= (nt - 1) u W', so
    |GIVE - ratio sum x| <= (nt - 1) u G' + u G, G' the sum of the magnitudes, which here are all >= 0: <= nt u G (1 + ..).  A cell's got
    is the rounded sum of at most NDEP rounded products x ratio: |got - sum x ratio| <= (NDEP + NDEP - 1) u got.  Both use the same
    doubles x and ratio, so |sum GIVE - sum TAKE| <= 1.01 u (ntmax sum GIVE + 2 NDEP sum TAKE), which is the bound of the second figure
    and enters the first."""
    down, up, area, p, _, tab, cmd, _, _ = forest
    state = _start(forest)
    res0 = state[3]
    ntmax = int(np.diff(cmd["ptr"]).max())
    with_terms = cmd["dams"][np.diff(cmd["ptr"]) > 0]
    total, worst, bound, gt, low = Fraction(0), Fraction(0), 0.0, 0.0, np.inf
    for c in range(ncall):
        wh, wt, volr, res = state[:4]
        out, (qin, qsur, wd) = _call(forest, state, c, variant=variant)
        wh1, wt1, v1, qout, res1, krls1, rtake, qin1 = out[:8]
        want, take, give, ratio = out[-4:]
        so = _fsum(qout[down < 0])
        r = ((_fsum(wh1) + _fsum(wt1) + _fsum(v1) + _fsum(res1)) - (_fsum(wh) + _fsum(wt) + _fsum(volr) + _fsum(res))
             - Fraction(DT) * (_fsum(qin1) - so) + _fsum(rtake) + _fsum(give))
        total += r
        worst = max(worst, abs(total))
        q = float(np.abs(qsur).sum() + np.abs(qin1 - qsur).sum())
        sc = float(wh.sum() + wt.sum() + volr.sum() + np.abs(res).sum()) + DT * q
        sq = float(np.abs(qin1).sum())
        b_gt = 1.01 * U * (ntmax * float(give.sum()) + 2 * rt.NDEP * float(take.sum()))
        bound += 1.01 * U * (17 * NSUB * sc + 5 * DT * q + (NSUB + 1) * NSUB * sc + DT * (sq + float(so)) + 8 * NSUB * sc + sc
                             + sc + float(take.sum()) + DT * sq) + b_gt
        gt = max(gt, float(abs(_fsum(give) - _fsum(take))) / b_gt)
        low = min(low, float((res1 - np.minimum(tab["SMIN"], res0))[with_terms].min()))
        state = _next(out)
    return float(worst), bound, gt, low


def test_mass_closure_in_exact_arithmetic(forest):
    """Over 30 calls the accumulated residual of C5's closure stays below the bound counted in _closure, every call's sum GIVE and
    sum TAKE agree inside theirs, and no dam with terms ends a call below min(SMIN, its first RES)."""
    res, bound, gt, low = _closure(forest, 30)
    print(f"closure: residual {res:.3e} m3, bound {bound:.3e}; |sum GIVE - sum TAKE| at most {gt:.3f} of its bound; RES - min(SMIN, RES0) >= {low:.3e}")
    assert res <= bound
    assert gt <= 1.0
    assert low >= 0.0


def test_the_wrong_variants_differ_and_fail_the_checks(forest):
    """The statement held against five wrong statements.  Each gives other bits on the case set, and:
      - QIN not credited: what the dams gave reaches no channel - the cells' QIN is short of sum TAKE, and WT with it;
      - avail without SMIN: a dam is drawn below min(SMIN, its first RES);
      - the allotment from the RES before D2's own take: the same (the dam promises what its own cell has just taken);
      - terms summed in reverse, and the ratio applied to WANT and not to the term: the same water, other roundings - inside the
        bounds, but not the bits (GIVE's and TAKE's)."""
    state = _start(forest)
    true, _ = _call(forest, state, 0)
    for v in rt.CMD_VARIANTS:
        out, _ = _call(forest, state, 0, variant=v)
        differ = [k for k in (2, 4, 7, -3, -2, -1) if bits(out[k]) != bits(true[k])]
        assert differ, v
    assert bits(_call(forest, state, 0, variant="reverse")[0][-2]) != bits(true[-2])  # GIVE
    good = _closure(forest, 5)
    assert good[0] <= good[1] and good[2] <= 1.0 and good[3] >= 0.0
    assert bits(_call(forest, state, 0, variant="ratio_on_want")[0][-3]) != bits(true[-3])  # TAKE
    lost, _ = _call(forest, state, 0, variant="no_credit")
    missing = float(((true[7] - lost[7]) * DT).sum())
    assert missing == pytest.approx(float(true[-3].sum()), rel=1e-12) and missing > 1.0e5 and float(lost[1].sum()) < float(true[1].sum())
    assert _closure(forest, 5, variant="no_smin")[3] < 0.0
    assert _closure(forest, 5, variant="before_d2")[3] < 0.0
    for v in ("reverse", "ratio_on_want"):
        other = _closure(forest, 5, variant=v)
        assert other[0] <= other[1] and other[2] <= 1.0


# ---- 4. a dam above a dry crop cell ---------------------------------------------------------------------------------------------------------
def test_two_days_on_a_chain_with_and_without_the_part():
    """A chain of four cells, a full reservoir at the top and a crop cell at the bottom whose channel (VOLR + WT, 2e4 m3) holds less than
    a day's demand (1.7e5 m3), hourly calls through two days.  With the part on the crop cell's VOLR stays above zero, its tributary
    store never goes negative, sum TAKE > 0 and the reservoir falls by what it gave; without it the withdrawal drives the cell's
    tributary store - and with it the cell's channel water, WT + VOLR - below zero."""
    down, area, p, (cap, target, beta, mstart, res0, krls0), rows, rn, i = cc.dry_chain()
    crop = 3
    up = rt.upstream_map(down)
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    cmd = rt.command_tables(cap, *rows)
    with np.errstate(all="ignore"):
        qin = ((rn - i) * 0.001) * area
    qsur = np.zeros(4)
    results = {}
    for on in (True, False):
        wh, wt, volr, res, krls = np.zeros(4), np.full(4, 1.0e4), np.full(4, 1.0e4), res0, krls0
        took, lowest_v, lowest_w = 0.0, np.inf, np.inf
        for _ in range(48):
            dam = {"tab": tab, "res": res, "krls": krls, "month": 6, "begins": False, "withdrawal": (rn, i)}
            if on:
                dam["command"] = cmd
            out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, 3600.0, 4, dam=dam)
            wh, wt, volr, res, krls = out[0], out[1], out[2], out[4], out[5]
            if on:
                took += float(out[-3].sum())
            lowest_v, lowest_w = min(lowest_v, float(volr[crop])), min(lowest_w, float(wt[crop]))
        results[on] = (lowest_v, lowest_w, float(wt[crop] + volr[crop]), took, float(res[0]))
    v, w, _, took, res_on = results[True]
    assert v > 0.0 and w >= 0.0 and took > 0.9 * 2.0 * 86400.0 * 2.0
    assert res_on < results[False][4] - 0.9 * took
    _, w, channel, _, _ = results[False]
    assert w < 0.0 and channel < 0.0


# ---- 5. the supply limit (C6) -----------------------------------------------------------------------------------------------------------------
def test_supply_limit_counts_the_claimed_storage():
    """Three cells of one column each: cell 0 a dam, cells 1 and 2 limited cells that hang on it, cell 2 with a claim of 0.  The ratio
    of cell 1 rises by exactly claim * (RES - SMIN) / Vd; cell 2 and the dam's own cell keep D7's ratio; with RES below SMIN nothing
    is added; without the part every cell keeps D7 / S3."""
    ptr, col, w = np.array([0, 1, 2, 3]), np.array([0, 1, 2], np.int32), np.ones(3)
    area, volr = np.full(3, 1.0e6), np.array([100.0, 100.0, 100.0])
    cap = np.array([1.0e4, 0.0, 0.0])
    tab = rt.reservoir_tables(cap, np.zeros((12, 3)), np.ones(3), np.zeros(3, np.int32))
    dam = np.full((4, 3), -1)
    share, claim = np.zeros((4, 3)), np.zeros((4, 3))
    dam[0, 1], share[0, 1], claim[0, 1] = 0, 1.0, 0.25
    dam[0, 2], share[0, 2], claim[0, 2] = 0, 0.5, 0.0
    cmd = rt.command_tables(cap, dam, share, claim)
    idt = 1800
    nspd = (ir.IRRIG_LENGTH + idt - 1) // idt
    rate, nleft = np.full(3, 1.0e-4), np.full(3, float(nspd))
    args = (ptr, col, w, area, volr, rate, nleft, idt, 0.0, np.zeros(3))
    res = np.array([5000.0, 0.0, 0.0])
    _, plain = ir.supply_limit(*args, dam=(tab, res))
    _, got = ir.supply_limit(*args, dam=(tab, res), command=cmd)
    vd = plain[ir.DEMAND]
    assert (vd > 100.0).all() and (plain[ir.RATIO][1:] < 1.0).all() and plain[ir.RATIO][0] == 1.0
    r = res[0] - tab["SMIN"][0]
    assert r == 4000.0
    assert got[ir.RATIO][1] == (100.0 + 0.25 * r) / vd[1] and got[ir.RATIO][1] * vd[1] - plain[ir.RATIO][1] * vd[1] == pytest.approx(0.25 * r, rel=1e-15)
    assert bits(got[ir.RATIO][[0, 2]]) == bits(plain[ir.RATIO][[0, 2]])
    low = np.array([900.0, 0.0, 0.0])
    assert bits(ir.supply_limit(*args, dam=(tab, low), command=cmd)[1]) == bits(ir.supply_limit(*args, dam=(tab, low))[1])
    for bad in (NAN, -INF):
        edge = np.array([bad, 0.0, 0.0])
        assert bits(ir.supply_limit(*args, dam=(tab, edge), command=cmd)[1][ir.RATIO][1:]) == bits(plain[ir.RATIO][1:] * 0.0 + 100.0 / vd[1:])
    with pytest.raises(ValueError):
        ir.supply_limit(*args, command=cmd)


# ---- 6. the check ---------------------------------------------------------------------------------------------------------------------------
def _valid(n=12):
    """tests/c/command_checks.cc: valid()."""
    cap = np.zeros(n)
    cap[2], cap[5], cap[9] = 1.0e9, 5e-324, 3.0e7
    dam, share, claim = np.full((4, n), -1, np.int64), np.full((4, n), NAN), np.full((4, n), -7.0)
    for k, c, d, s, q in ((0, 0, 2, 0.5, 0.25), (1, 0, 5, 0.5, 1.0), (0, 1, 5, 1.0, 0.0), (0, 5, 2, 0.125, 0.25), (0, 7, 5, 0.375, 0.0),
                          (1, 7, 2, 0.0625, 0.5)):
        dam[k, c], share[k, c], claim[k, c] = d, s, q
    return cap, dam, share, claim


def _cases():
    """The cases of tests/c/command_checks.cc that reach the rows: name -> (cap, dam, share, claim)."""
    out = {}

    def case(name, edit, n=12):
        cap, dam, share, claim = _valid(n)
        edit(cap, dam, share, claim)
        out[name] = (cap, dam, share, claim)

    def put(k, c, d, s, q):
        def edit(cap, dam, share, claim):
            dam[k, c], share[k, c], claim[k, c] = d, s, q
        return edit

    def assign(row, k, c, v):
        def edit(cap, dam, share, claim):
            {"dam": dam, "share": share, "claim": claim}[row][k, c] = v
        return edit

    def both(*edits):
        def edit(*a):
            for e in edits:
                e(*a)
        return edit

    for b, v in enumerate((-2, 12, 2 ** 31 - 1, -2 ** 31)):
        case(f"bad index {b}", assign("dam", 1, 1, v))
    case("gap", put(2, 1, 2, 0.5, 0.0))
    case("no reservoir", put(1, 1, 3, 0.5, 0.0))
    case("itself", put(1, 5, 5, 0.5, 0.0))
    case("twice", put(2, 7, 5, 0.25, 0.0))
    for b, v in enumerate((0.0, -0.5, 1.0000000000000002, NAN, INF)):
        case(f"bad SHARE {b}", assign("share", 1, 7, v))
    for b, v in enumerate((-1.0e-9, 1.0000000000000002, NAN, INF)):
        case(f"bad CLAIM {b}", assign("claim", 0, 5, v))
    case("shares above 1", assign("share", 1, 0, 0.5000000000000002))
    case("claims above 1", assign("claim", 1, 7, 0.5000000000000002))
    case("cells before dams", both(assign("claim", 1, 7, 0.5000000000000002), assign("share", 0, 1, 2.0)))
    case("first cell", both(assign("share", 0, 7, 0.0), assign("share", 0, 1, NAN)))
    case("valid", lambda *a: None)
    case("sixty-five cells", put(0, 64, 9, 1.0, 1.0), n=65)
    case("no dependents", lambda cap, dam, share, claim: dam.fill(-1))

    def no_dams(cap, dam, share, claim):
        dam.fill(-1)
        cap.fill(0.0)
    case("no dams", no_dams)
    return out


def _line(cap, dam, share, claim, show=True):
    """What command_checks.cc prints behind "<case>: " for these inputs, from the Python side."""
    try:
        t = rt.command_tables(cap, dam, share, claim)
    except ValueError as e:
        return str(e)
    terms = "".join(f" {c}/{k}/{float(s).hex()}" for c, k, s in zip(t["cell"], t["slot"], t["share"]))
    return "ok dams" + "".join(f" {d}" for d in t["dams"]) + " ptr" + "".join(f" {q}" for q in t["ptr"]) + " terms" + terms


EXPECTED_TEXT = {"bad index 0": rt.E_CMD_RANGE, "gap": rt.E_CMD_GAP, "no reservoir": rt.E_CMD_NODAM, "itself": rt.E_CMD_SELF, "twice": rt.E_CMD_TWICE,
                 "bad SHARE 3": rt.E_CMD_SHARE, "bad CLAIM 2": rt.E_CMD_CLAIM, "shares above 1": rt.E_CMD_SHARE_SUM,
                 "claims above 1": rt.E_CMD_CLAIM_SUM}


def test_check_command_names_the_row_and_the_first_cell():
    cases = _cases()
    for name, text in EXPECTED_TEXT.items():
        with pytest.raises(ValueError) as e:
            rt.check_command(*cases[name])
        assert str(e.value).startswith(text + " at cell "), name
    assert _line(*cases["claims above 1"]) == rt.e_cell(rt.E_CMD_CLAIM_SUM, 2)  # the dam's cell
    assert _line(*cases["first cell"]) == rt.e_cell(rt.E_CMD_SHARE, 1) and _line(*cases["cells before dams"]) == rt.e_cell(rt.E_CMD_SHARE, 1)
    rt.check_command(*cases["valid"])
    t = rt.command_tables(*cases["valid"])
    assert t["dams"].tolist() == [2, 5, 9] and t["ptr"].tolist() == [0, 3, 6, 6]
    assert list(zip(t["cell"].tolist(), t["slot"].tolist())) == [(0, 0), (5, 0), (7, 1), (0, 1), (1, 0), (7, 0)]
    assert not t["SHARE"][t["DAM"] < 0].any() and not t["CLAIM"][t["DAM"] < 0].any() and t["HAS"].tolist() == [c in (0, 1, 5, 7) for c in range(12)]
    with pytest.raises(ValueError, match="must be"):
        rt.check_command(np.zeros(5), np.full((4, 6), -1), np.zeros((4, 6)), np.zeros((4, 6)))
    # a tie that rounds down is inside the limit: 0.5 + (0.5 + 2^-53) == 1.0
    cap, dam, share, claim = _valid()
    share[1, 0] = 0.5000000000000001
    rt.check_command(cap, dam, share, claim)


def _build_checks(tmp_path, flags, name):
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "c", name + ".cc")
    inc = os.path.join(ROOT, "elmkernels_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan-ubsan"])
def test_the_host_check_as_a_program(tmp_path, flags):
    """tests/c/command_checks.cc drives elmk_maps.h: command_check: every refusal with the text and the cell check_command gives, the
    inverse map bit for bit command_tables', padding cells and empty slots -1 and zero."""
    exe = _build_checks(tmp_path, flags, "command_checks")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    lines = dict(s.split(": ", 1) for s in out)
    assert lines["ncells 0"] == rt.E_NCELLS + " -1"
    assert all(lines[k] == "null argument" for k in ("null cap", "null dam", "null share", "null claim"))
    cases = _cases()
    assert set(cases) | {"ncells 0", "null cap", "null dam", "null share", "null claim"} == set(lines)
    def norm(line):  # (printf's %a and float.hex spell the same double differently)
        return " ".join("/".join(t.split("/")[:2] + [float.fromhex(t.split("/")[2]).hex()]) if t.count("/") == 2 else t for t in line.split(" "))

    for name, inputs in cases.items():
        assert norm(lines[name]) == _line(*inputs), name
    assert not any("BAD" in s for s in out)


def test_the_header_the_bindings_and_the_constants_agree():
    text = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert "enum { ELMK_ROUTE_CMD_WANT = 21, ELMK_ROUTE_CMD_TAKE = 22, ELMK_ROUTE_CMD_GIVE = 23, ELMK_ROUTE_CMD_RATIO = 24 };" in text
    assert "enum { ELMK_CMD_NDEP = 4 };" in text
    assert (rt.CMD_WANT, rt.CMD_TAKE, rt.CMD_GIVE, rt.CMD_RATIO) == (st.ROUTE_CMD_WANT, st.ROUTE_CMD_TAKE, st.ROUTE_CMD_GIVE, st.ROUTE_CMD_RATIO) == (21, 22, 23, 24)
    assert rt.NDEP == st.ROUTE_CMD_NDEP == 4 == cc.NDEP
    maps = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    for t in (rt.E_CMD_RANGE, rt.E_CMD_GAP, rt.E_CMD_NODAM, rt.E_CMD_SELF, rt.E_CMD_TWICE, rt.E_CMD_SHARE, rt.E_CMD_CLAIM, rt.E_CMD_SHARE_SUM,
              rt.E_CMD_CLAIM_SUM):
        assert f'"{t}"' in maps, t
    kern = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_routing.hip")).read()
    assert f"CMD_DAMS = {cc.CMD_DAMS}, CMD_TILE = {cc.CMD_TILE}" in kern
