"""The irrigation's edge tier on the host (tests/irrigation_cases.py: edge_tier; tests/irrigation_supply_cases.py: edge_rows,
shape_map): what makes the device tests of tests/test_gpu_irrigation_edges.py non-vacuous, and an independent check of the
restatement they compare with.  The census of the tier is complete on irrigation.step alone at every step length; the clock against a
brute-force scan of the step's seconds; the window's step count over every whole step length; irrigation.check_rate on the edge
values against the formula in plain floats and against a by-value table of what include/elmk.h's statement implies; wrong variants of
the statement, each of which changes a bit of the tier's results; the limit's finite cells against exact arithmetic.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import irrigation as ir
from tests import irrigation_cases as IC
from tests import irrigation_supply_cases as SC
from tests.support import bits

NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53
N = 257  # holds every edge class once


# ---- the chain both sides run ---------------------------------------------------------------------------------------------------------
def _chain(dt, stored=None, seen=None, n=N):
    """The edge tier through the chain of clock_tods(dt), the two state fields carried from call to call as a context carries them:
    the rows after every call and the two fields after the last."""
    cols, _, _, sched = IC.edge_tier(n, 900)
    smpso = IC.smpso_of(cols["vtype"])
    with np.errstate(over="ignore"):
        f = {k: (np.asarray(cols[k]).astype(stored) if stored is not None and cols[k].dtype == np.float64 else np.array(cols[k])) for k in ir.READS}
    rate, nleft = IC.edge_seed(n, dt)
    rows = np.stack([rate, nleft, np.zeros(n)])
    seen = {} if seen is None else seen
    out = []
    for tod in IC.clock_tods(dt):
        fields, rows = IC.edge_step(seen, f, rows, sched, float(dt), tod, smpso, stored=stored)
        f.update(fields)
        out.append(rows)
    return np.array(out), {k: f[k] for k in ir.WRITES}


@pytest.mark.parametrize("stored", [None, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("dt", IC.DTS)
def test_the_census_is_complete_on_the_restatement(dt, stored):
    """Every name of EDGE_CENSUS is met at 257 columns over the chain of clock_tods(dt), in the values either build stores.  At a step
    of a day off_clock and since_first_out are exempt (census_missing says why); at dt = 1 a window of 14400 steps cannot run out in
    a chain of eight calls, and window_ran_out comes from the seeded NLEFT 1 and 2."""
    seen = {}
    rows, _ = _chain(dt, stored, seen)
    print(f"dt={dt} census: {seen}")
    assert not IC.census_missing(seen, dt), IC.census_missing(seen, dt)
    assert set(seen) == set(IC.EDGE_CENSUS)
    if dt == 86400:
        assert not seen["off_clock"] and not seen["since_first_out"]  # (the exemption is no oversight: they cannot occur)
    assert np.isnan(rows[-1][ir.RATE]).any() and (rows[-1][ir.RATE] == INF).any()  # what the limit's sums meet behind such a call


def test_the_tier_lays_out_every_class_and_mixes_a_wave():
    classes = IC.edge_classes()
    assert 2 * len(classes) - 1 <= N and len({c[0] for c in classes}) == len(classes)
    assert sum(1 for c in classes if c[1] != "apply") == len(IC.EDGE_SLOTS) * len(IC.EDGE_VALUES) + 7 + 1  # (with the smpso = 0 type)
    cols, _, _, sched = IC.edge_tier(N, 900)
    assert IC.smpso_of(cols["vtype"])[IC.edge_index("smpso=0", N)] == 0.0
    assert set(sched[1::2].tolist()) == set(IC.CLOCK_SCHED) | {-1} and (sched[0:2 * len(classes):2] == 0).all()
    rate, nleft = IC.edge_seed(N, 1800)
    k = [IC.edge_index(f"apply{i}", N) for i in range(IC.N_APPLY)]
    assert {(nleft[i], rate[i]) for i in k} == {(a, b) for a in (1.0, 2.0, 8.0) for b in IC.APPLY_RATE}
    assert len({(int(cols["do_capsnow"][i]), bits(np.float64(cols["qflx_snwcp_liq" if cols["do_capsnow"][i] else "qflx_rain_grnd"][i]))) for i in k}) == 20
    # one column alone is an edge column that checks
    c1, _, _, s1 = IC.edge_tier(1, 900)
    seen = {}
    IC.edge_step(seen, {k: c1[k] for k in ir.READS}, np.zeros((3, 1)), s1, 1800.0, IC.clock_tods(1800)[0], IC.smpso_of(c1["vtype"]))
    assert seen["check"] == 1
    # in the first wave of the first call some columns check, some apply and some do neither
    rows = np.stack([rate, nleft, np.zeros(N)])
    _, after = ir.step({k: cols[k] for k in ir.READS}, rows, sched, 1800.0, IC.clock_tods(1800)[0], IC.smpso_of(cols["vtype"]))
    checked, applied = (after[ir.NLEFT] == 8.0)[:64], (nleft > 0.0)[:64]
    assert checked.any() and applied.any() and (~checked & ~applied).any()


# ---- the clock ------------------------------------------------------------------------------------------------------------------------
CLOCK_SCHEDS = (0, 1, 21599, 21600, 21601, 64800, 86399)


@pytest.mark.parametrize("idt", IC.DTS)
def test_the_clock_against_a_scan_of_the_steps_seconds(idt):
    """B's clock in other words (include/elmk.h: since = the seconds the local clock is past 06:00 at the step's start, and the
    column checks with since < idt): a column checks in the step before whose start its local 06:00:00 came by less than a step -
    some second s of (tod - idt, tod] has (s + sched) % 86400 == 21600.  So the step that starts at 06:00:00 local checks, the step
    that starts idt - 1 seconds later checks and the one that starts idt seconds later does not.  The scan marks every second of
    three days that is a local 06:00:00 and counts the marks among each step's idt seconds (a running count: every tod of the day
    at every step length); a literal loop over the seconds does the same for a stride of tods and the day's boundaries.  Neither
    shares anything with `since < idt`."""
    day = ir.DAY
    for sched in CLOCK_SCHEDS:
        s = np.arange(3 * day)
        mark = ((s + sched) % day == 21600).astype(np.int64)
        run = np.concatenate([[0], np.cumsum(mark)])
        tod = np.arange(day)
        want = (run[day + tod + 1] - run[day + tod + 1 - idt]) > 0  # the seconds day + tod - idt + 1 .. day + tod
        # seconds_since_start takes one tod and a row of sched; a column of sched s at tod t has the local clock of a column of
        # sched (t + s) % 86400 at tod 0, which gives every tod of the day in one call (six of them are checked as step calls it)
        since = ir.seconds_since_start((tod + sched) % day, 0)
        for t in (0, 1, 21599, 21600, 43200, 86399):
            assert int(ir.seconds_since_start(np.array([sched]), t)[0]) == int(since[t]), (sched, t)
        got = since < idt
        assert (got == want).all(), (idt, sched, np.nonzero(got != want)[0][:5])
        assert int(want.sum()) == min(idt, day)
        stride = list(range(0, day, 4999)) + [21599 - sched, 21600 - sched, 21600 - sched + idt - 1, 21600 - sched + idt, 0, day - 1]
        for t in (x % day for x in stride):
            literal = any((sec + sched) % day == 21600 for sec in range(t - idt + 1, t + 1))
            assert literal == bool(int(ir.seconds_since_start(np.array([sched]), t)[0]) < idt), (idt, sched, t)


def test_the_windows_step_count_over_every_whole_step_length():
    """nspd steps cover the four hours and nspd - 1 do not: nspd * dt >= 14400 > (nspd - 1) * dt, for every dt in 1 .. 86400."""
    for dt in range(1, ir.DAY + 1):
        nspd = ir.steps_per_day(dt)
        assert nspd * dt >= 14400 > (nspd - 1) * dt, dt
    assert [ir.steps_per_day(dt) for dt in IC.DTS] == [14400, 8, 4, 3, 1, 1, 1]


# ---- check_rate on the edge values ------------------------------------------------------------------------------------------------------
def _column_lists(cols, c):
    s0 = ir.NLEVSNO
    g = lambda k, lo: np.asarray(cols[k][c], dtype=np.float64)[lo:lo + ir.NLEVGRND].tolist()  # noqa: E731
    return g("t_soisno", s0), g("rootfr", 0), g("eff_porosity", 0), g("sucsat", 0), g("bsw", 0), g("dz", s0), g("h2osoi_liq", s0)


def test_check_rate_on_the_edge_columns_equals_the_formula_in_plain_floats():
    """Every edge column through irrigation.check_rate and through rate_by_hand (Python's own pow, / and max over the layers above the
    first one with t <= tfrz).  Python raises where IEEE gives an infinity or a NaN (a division by zero, 0 to a negative power, a
    negative base): those columns are the by-value table's below; all the others - the majority, NaN and infinite results among
    them - agree bit for bit."""
    cols, _, _, _ = IC.edge_tier(N, 900)
    smpso = IC.smpso_of(cols["vtype"])
    compared = raised = nonfinite = 0
    for k, (name, *_rest) in enumerate(IC.edge_classes()):
        c = 2 * k
        lists = _column_lists(cols, c)
        frozen = [j for j, t in enumerate(lists[0]) if t <= ir.TFRZ]
        for dt in (1, 7000, 86400):
            got = ir.check_rate(*lists, float(smpso[c]), float(dt) * ir.steps_per_day(dt))
            try:
                want = IC.rate_by_hand(cols, c, frozen[0] if frozen else 15, float(dt), float(smpso[c]))
            except (ZeroDivisionError, ValueError, OverflowError):
                raised += 1
                continue
            want = NAN if want != want else want
            assert bits(np.float64(got)) == bits(np.float64(want)), (name, dt, got, want)
            compared += 1
            nonfinite += not math.isfinite(got)
    print(f"compared {compared}, Python raised in {raised}, non-finite results compared {nonfinite}")
    assert compared > 4 * raised and nonfinite > 20


def _rate(dtn=14400.0, smpso=-66000.0, **over):
    """check_rate on one loam column (eff_porosity 0.45, sucsat 200, bsw 5, dz 0.1, 20 mm of water, 280 K, roots in layers 0 .. 9) with
    `over`: name -> (layer, value)."""
    v = {"t": [280.0] * 15, "rootfr": [0.1] * 10 + [0.0] * 5, "effpor": [0.45] * 15, "sucsat": [200.0] * 15, "bsw": [5.0] * 15, "dz": [0.1] * 15,
         "liq": [20.0] * 15}
    for k, (j, x) in over.items():
        v[k][j] = x
    return ir.check_rate(v["t"], v["rootfr"], v["effpor"], v["sucsat"], v["bsw"], v["dz"], v["liq"], smpso, dtn)


def test_the_edge_values_do_what_the_statement_says():
    """By value, from include/elmk.h "irrigation" B: `t <= tfrz` breaks, so a NaN or +inf temperature does not and -inf or exactly tfrz
    does; `rootfr > 0.0` measures, so a NaN, zero or negative root fraction skips the layer; every operation of a measured layer
    passes a NaN on and max(a, b) = (a < b ? b : a) keeps a NaN deficit, so a NaN anywhere in a rooted thawed layer gives the
    canonical NaN rate; h2osoi_liq = -inf gives deficit +inf and h2osoi_liq = +inf gives deficit 0."""
    full = _rate()
    ten = [_rate(t=(j, 0.0)) for j in range(11)]  # the rate of layers 0 .. j - 1
    assert ten[0] == 0.0 and not math.copysign(1.0, ten[0]) < 0 and ten[10] == full and all(a < b for a, b in zip(ten[:10], ten[1:11]))
    # the temperature
    for j in (0, 3, 9):
        assert _rate(t=(j, NAN)) == full and _rate(t=(j, INF)) == full and _rate(t=(j, 1e300)) == full
        assert _rate(t=(j, float(np.nextafter(ir.TFRZ, INF)))) == full
        for cold in (-INF, ir.TFRZ, -0.0, -3.5, 5e-324):
            assert bits(np.float64(_rate(t=(j, cold)))) == bits(np.float64(ten[j])), (j, cold)
    # the root fraction: a layer is measured only for rootfr > 0.0
    skipped = _rate(rootfr=(2, 0.0))
    assert skipped < full
    for r in (NAN, -0.0, -3.5, -INF):
        assert bits(np.float64(_rate(rootfr=(2, r)))) == bits(np.float64(skipped)), r
    for r in (5e-324, 1e300, INF):
        assert _rate(rootfr=(2, r)) == full, r  # (its size does not enter the formula)
    # a NaN in a measured layer
    for name in ("effpor", "sucsat", "bsw", "dz", "liq"):
        got = np.float64(_rate(**{name: (2, NAN)}))
        assert got.view(np.uint64) == 0x7FF8000000000000, name
        assert _rate(**{name: (12, NAN)}) == full and _rate(t=(1, 0.0), **{name: (2, NAN)}) == ten[1]  # rootless; below a frozen layer
    assert np.float64(_rate(smpso=NAN)).view(np.uint64) == 0x7FF8000000000000
    # the water held
    assert _rate(liq=(2, -INF)) == INF
    dry = _rate(liq=(2, INF))
    assert dry == _rate(liq=(2, 1e300)) and 0.0 < full - dry and abs((full - dry) - (ten[3] - ten[2])) <= 4 * U * full
    # a suction of 0 or below, an exponent's denominator of 0: IEEE's values, never an exception
    assert np.isnan(_rate(sucsat=(2, -3.5)))  # pow of a negative base with a fractional exponent
    # sucsat = +0 and -0: the base is +inf and -inf, and pow(+-inf, -0.2) = +0 - the wilting-point water is 0, as with bsw = +0 below
    assert _rate(sucsat=(2, 0.0)) == _rate(sucsat=(2, -0.0)) == _rate(bsw=(2, 0.0)) and math.isfinite(_rate(sucsat=(2, 0.0)))
    assert np.isnan(_rate(smpso=0.0)) and math.isfinite(_rate(bsw=(2, INF))) and math.isfinite(_rate(bsw=(2, -INF)))
    assert _rate(bsw=(2, 0.0)) == _rate(bsw=(2, 5e-324))  # -1 / +0 and -1 / 5e-324 are both -inf: pow(330, -inf) = 0
    assert np.isnan(_rate(bsw=(2, -0.0)))  # pow(330, +inf) = +inf: liq_so +inf, liq_sat - liq_so -inf, their sum NaN
    assert _rate(dz=(2, 0.0)) == skipped and _rate(dz=(2, -3.5)) == skipped  # the deficit is -liq, or negative: max gives 0
    assert np.isnan(_rate(dz=(2, INF))) and np.isnan(_rate(effpor=(2, INF)))  # inf - inf


# ---- wrong variants ---------------------------------------------------------------------------------------------------------------------
def _supply_side(dt, thr=0.1, drop_y=False, clamp=False):
    """edge_rows on a map of 80 cells through irrigation.supply_limit.  drop_y: without S2's y; clamp: NLEFT > nspd handed over as
    nspd, which marks the columns `NLEFT >= nspd` would mark."""
    ncols, ncells = 900, 80
    ptr, col, w = SC.cell_map(ncols, ncells, 41, big=(3, 90), empty=(0, 30, 31, 32, 33), single=(5, 7))
    area, volr = SC.cell_values(ncells, 42, lo=4.0, hi=7.5)
    nspd = ir.steps_per_day(dt)
    rate, nleft, qirr, volr = SC.edge_rows(ptr, col, ncols, nspd, 43, volr)
    unmet = np.random.default_rng(44).uniform(0.0, 1.0e5, ncells)
    if clamp:
        nleft = np.where(nleft >= float(nspd), float(nspd), nleft)
    r, rows = ir.supply_limit(ptr, col, w, area, volr, rate, nleft, dt, thr, unmet, qflx_irrig=None if drop_y else qirr)
    return (ptr, col, w, area, volr, rate, nleft, qirr, unmet, ncols), r, rows


def _results(dt, **kw):
    rows, fields = _chain(dt)
    _, r, sup = _supply_side(dt, **kw)
    return bits(rows) + b"".join(bits(fields[k]) for k in ir.WRITES) + bits(r) + bits(sup)


@pytest.fixture(scope="module")
def right():
    return {dt: _results(dt) for dt in IC.DTS}


def _check_rate_variant(lt=False, fmax=False):
    def check_rate(t, rootfr, effpor, sucsat, bsw, dz, liq, smpso, dtn, hit=None):
        rate = 0.0
        for j in range(ir.NLEVGRND):
            if (t[j] < ir.TFRZ) if lt else (t[j] <= ir.TFRZ):
                break
            if rootfr[j] > 0.0:
                vol_liq_so = effpor[j] * ir._pow(ir._div(-smpso, sucsat[j]), ir._div(-1.0, bsw[j]))
                liq_so = vol_liq_so * ir.DENH2O * dz[j]
                liq_sat = effpor[j] * ir.DENH2O * dz[j]
                d = (liq_so + ir.IRRIG_FACTOR * (liq_sat - liq_so)) - liq[j]
                deficit = (0.0 if d != d else max(d, 0.0)) if fmax else ir._max(d, 0.0)
                rate = rate + ir._div(deficit, dtn)
        return NAN if rate != rate else rate
    return check_rate


def _fmax(a, b):
    return b if a != a else (a if b != b else (b if a < b else a))


VARIANTS = ("since_le_idt", "nspd_floor", "t_lt_tfrz", "fmax_for_max", "nleft_ge_nspd", "committed_without_y")


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_wrong_variant_changes_a_bit(variant, right, monkeypatch):
    """One-character slips of the statement, put into the restatement at its seams, against the tier's results (the rows of every
    call of the chain, the two state fields, and RATE and the four cell rows of the limit on edge_rows) at every step length of DTS:
    each changes at least one bit at some step length.  `since <= idt`; floor for ceiling in nspd; `t < tfrz`; fmax (which drops a
    NaN) for max; `NLEFT >= nspd` in S0; the committed water without this step's y."""
    kw = {}
    if variant == "since_le_idt":
        real = ir.seconds_since_start
        monkeypatch.setattr(ir, "seconds_since_start", lambda sched, tod: real(sched, tod) - 1)
    elif variant == "t_lt_tfrz":
        monkeypatch.setattr(ir, "check_rate", _check_rate_variant(lt=True))
    elif variant == "fmax_for_max":
        monkeypatch.setattr(ir, "_max", _fmax)
    elif variant == "nleft_ge_nspd":
        kw["clamp"] = True
    elif variant == "committed_without_y":
        kw["drop_y"] = True
    changed = []
    for dt in IC.DTS:
        if variant == "nspd_floor":
            if dt > 14400:
                continue  # (floor gives nspd = 0 there)
            monkeypatch.setattr(ir, "IRRIG_LENGTH", 14400 - (dt - 1))  # (14400 - (idt - 1) + (idt - 1)) // idt: the floor
        if _results(dt, **kw) != right[dt]:
            changed.append(dt)
    print(variant, "changes a bit at dt in", changed)
    assert changed, variant
    if variant == "nspd_floor":
        assert 7000 in changed and 1800 not in changed  # (only where dt does not divide the window)
    if variant == "since_le_idt":
        assert 86400 not in changed and 1 in changed
    # the variant of the patched seam that takes the right form again gives the right bits (the patch itself is no change)
    if variant in ("t_lt_tfrz", "fmax_for_max"):
        monkeypatch.undo()
        monkeypatch.setattr(ir, "check_rate", _check_rate_variant())
        assert all(_results(dt) == right[dt] for dt in (1800, 7000))


# ---- the limit's finite cells against exact arithmetic ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [1, 7000, 86400])
def test_the_limits_finite_cells_against_exact_sums(dt):
    """DEMAND and COMMITTED of every cell whose terms are all finite against fractions.Fraction sums of the same terms.

    The bound, counted from the statement's roundings (u = 2^-53).  Every term is non-negative (rates, weights and areas are), so
    each partial result is at most the final one and a rounding of relative error u moves the result by at most u times the sum.
      a term of D   idt * NLEFT (1; exact in fact, a whole number below 2^53), RATE * that (1), w * d (1)                      3
      a term of C   the same two for e, QFLX_IRRIG * idt (1), e + y (1), w * c (1)                                            5
      a cell of m terms  the roundings of its terms act on the terms, each a part of the sum: together at most 3 u (5 u) of the
                    sum; m - 1 additions; S3's two scalings (* 0.001, * area)
    so |Vd - exact| <= (3 + (m - 1) + 2) u exact and |Vc - exact| <= (5 + (m - 1) + 2) u exact, times 1.01 for the higher orders.
    A result that underflows is rounded with an absolute error of at most 2^-1075 instead; what follows multiplies it by at most
    max(1, area) (w and 0.001 are below 1.5), and a cell has 5 m + (m - 1) + 2 roundings at most: that many times 2^-1075
    max(1, area) is added.  Where the exact sum is 2^1024 or more the row must hold +inf."""
    (ptr, col, w, area, volr, rate, nleft, qirr, unmet, ncols), _, rows = _supply_side(dt)
    nspd = ir.steps_per_day(dt)
    F = Fraction
    compared = overflowed = tiny = 0
    for c in range(area.size):
        terms = range(int(ptr[c]), int(ptr[c + 1]))
        cols_c = [int(col[p]) for p in terms]
        if not all(math.isfinite(rate[i]) and math.isfinite(qirr[i]) for i in cols_c):
            continue
        m = len(cols_c)
        d = e = F(0)
        for p, i in zip(terms, cols_c):
            x = F(float(rate[i])) * dt * int(nleft[i])
            checks = nleft[i] == float(nspd)
            d += F(float(w[p])) * (x if checks else 0)
            e += F(float(w[p])) * ((x if (not checks and nleft[i] > 0.0) else 0) + F(float(qirr[i])) * dt)
        k = F(0.001) * F(float(area[c]))
        for which, exact, per_term in ((ir.DEMAND, d * k, 3), (ir.COMMITTED, e * k, 5)):
            got = float(rows[which][c])
            if exact >= F(2) ** 1024:
                assert got == INF, (c, which)
                overflowed += 1
                continue
            bound = F(1.01 * (per_term + max(m - 1, 0) + 2) * U) * exact + (6 * m + 1) * F(2) ** -1075 * F(max(1.0, float(area[c])))
            assert math.isfinite(got) and abs(F(got) - exact) <= bound, (c, which, got, float(exact), float(bound))
            compared += 1
            tiny += 0 < exact < F(2) ** -1000
    print(f"dt={dt}: {compared} sums compared, {overflowed} overflow to +inf, {tiny} below 2^-1000")
    assert compared > 80 and overflowed > 0 and tiny > 0


def test_the_limits_edge_inputs_hold_every_edge_case():
    """edge_rows through irrigation.supply_limit, one call: every name of SUPPLY_EDGE_CASES but the two that need a workgroup of 64
    cells is met at every step length, and the earlier CASES still are."""
    for dt in IC.DTS:
        (ptr, col, w, area, volr, rate, nleft, qirr, unmet, ncols), r, rows = _supply_side(dt)
        nspd = ir.steps_per_day(dt)
        have = SC.supply_edge_census(ptr, col, ncols, nleft, rate, r, nspd, rows)
        missing = {k for k in SC.SUPPLY_EDGE_CASES if not have[k]}
        assert missing <= {"quiet_workgroup"}, (dt, missing)  # (80 cells: the first 64 hold the edge storages, the rest is ragged)
        old = SC.census(ptr, col, ncols, volr, nleft, rate, nspd, rows)
        gone = {k for k in SC.CASES if not old[k]}
        # at nspd = 1 no column is inside an open window (0 < NLEFT < nspd is empty): committed water is S2's y alone
        assert gone <= ({"mixed_cell"} if nspd == 1 else set()), (dt, gone)


@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 129])
def test_the_map_shapes_are_what_they_claim(ncells):
    for layout in SC.LAYOUTS:
        ptr, col, w, ncols = SC.shape_map(ncells, 7, layout)
        cnt = np.diff(ptr)
        assert ptr.size == ncells + 1 and np.unique(col).size == col.size and col.size == ptr[-1] and (w > 0.0).all()
        assert ncols - col.size >= 3 and (col.size == 0 or int(col.max()) < ncols)
        spans = [int(cnt[g:g + SC.SUP_CELLS].sum()) for g in range(0, ncells, SC.SUP_CELLS)]
        if layout == "tiles":
            assert spans[:2] == [SC.SUP_TILE, SC.SUP_TILE + 1][:len(spans)]
        elif layout == "big_last":
            assert int(cnt[min(ncells, 64) - 1]) == 2100 and spans[1:2] in ([], [0])
        else:
            assert not cnt.any()
    lead = [4, 10, 200]
    ptr, col, w, ncols = SC.shape_map(129, 7, "big_last", lead=lead)
    cell = SC.cell_of_column(ptr, col, ncols)
    assert [int(col[ptr[cell[i]]]) for i in lead] == lead and len({int(cell[i]) for i in lead}) == 3 and all(cell[i] >= 14 for i in lead)
