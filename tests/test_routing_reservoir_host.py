"""Reservoirs on the host (include/elmk.h "reservoirs"; elmkernels_amd/routing.py): the census of D1 - D3 and D2 on the inputs the
device test uses; no dams against the form without the extension; the statement held against wrong variants; D6's closure in exact
rational arithmetic against a bound counted from the statement's roundings; one dam through two years of a seasonal inflow; the
input check through a stand-alone program, plain and under the address and undefined-behaviour sanitizers; Hanasaki's rules; the
calendar; the header's constants and the bindings."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import reservoir_cases as rc
from tests.support import ROOT, bits

U = 2.0 ** -53
N = 1001


@pytest.fixture(scope="module")
def forest():
    """The 1001-cell forest of the device test with its cells, dams and (3, 1800 s) flood values, edge values taken out of the storages
    (the census and the closure are about finite water)."""
    ddist, area, p0, volr, wh, wt = rc.cell_values(N, 40 + N)
    rdepth, eprof, p, volr, wh, wt, wf = rc.flood_values(N, 60 + N, area, p0, volr, wh, wt, 3, 1800.0)
    fin = lambda x: np.where(np.isfinite(x) & (np.abs(x) < 1e200) & (x >= 0.0), x, 7.0)  # noqa: E731
    volr, wh, wt, wf = (fin(x) for x in (volr, wh, wt, wf))
    area = np.where(area > 0.0, area, 1.0e8)
    cap, target, beta, mstart, res, krls = rc.dam_values(N, 90 + N)
    for lo, edges in ((rc.RES_EDGE0, rc.SPECIAL), (rc.CAP_EDGE0, rc.CAP_EDGES)):
        for i in range(len(edges)):
            cap[lo + 2 * i], res[lo + 2 * i] = 1.0e9, 4.0e8
    down = rc.networks(N, 52 + N)["forest"]
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    ftab = rt.inundation_tables(area, p, rdepth, eprof)
    return down, rt.upstream_map(down), area, p, (wh, wt, volr, wf), tab, ftab, res, krls


def _inputs(area, call):
    rn, i = rc.aggregates(N, 5, call)
    with np.errstate(all="ignore"):
        qin = ((rn - i) * 0.001) * area
    return qin, 0.3 * np.abs(qin), (rn, i)


# ---- 1. the census --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flood", [False, True], ids=["plain", "flood"])
def test_every_branch_is_taken_in_every_call(forest, flood):
    """Five chained calls on the forest with the withdrawal on, `begins` on call 3: every branch of D3 and D2 is taken by at least one
    dam cell in every call, and D1 by at least one cell in call 3 and by none in any other."""
    down, up, area, p, (wh, wt, volr, wf), tab, ftab, res, krls = forest
    dt, nsub = 1800.0, 3
    for c in range(rc.NCALLS):
        month, begins = rc.call_time(c)
        qin, qsur, wd = _inputs(area, c)
        dam = {"tab": tab, "res": res, "krls": krls, "month": month, "begins": begins, "withdrawal": wd}
        seen = rc.call_census(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, dam, flood=(ftab, wf) if flood else None)
        missing = [k for k in rt.DAM_BRANCHES if not seen[k].any()]
        assert not missing, (c, missing)
        assert seen["D1"].any() == (c == rc.BEGINS_CALL)
        out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, flood=(ftab, wf) if flood else None, dam=dam)
        wh, wt, volr = out[:3]
        if flood:
            wf = out[4]
        res, krls, take = out[-4], out[-3], out[-2]
        assert (take[tab["DAM"]] > 0.0).any() and not take[~tab["DAM"]].any()
        if c == rc.BEGINS_CALL:
            assert bits(krls) != bits(dam["krls"])
        else:
            assert bits(krls) == bits(dam["krls"])


# ---- 2. no dams -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flood", [False, True], ids=["plain", "flood"])
def test_no_dams_give_the_bits_of_the_form_without_the_extension(forest, flood):
    """cap == 0 everywhere: all rows of kinematic_call without dam, bit for bit, with the edge values in the storages; RES and KRLS keep
    what they held, RES_TAKE is zero and QIN is K1's."""
    down, up, area, p, _, _, _, res, krls = forest
    ddist, area0, p0, volr, wh, wt = rc.cell_values(N, 40 + N)
    rdepth, eprof, p, volr, wh, wt, wf = rc.flood_values(N, 60 + N, area0, p0, volr, wh, wt, 3, 1800.0)
    ftab = rt.inundation_tables(area0, p, rdepth, eprof)
    tab = rt.reservoir_tables(np.zeros(N), np.full((12, N), rc.NAN), np.full(N, 7.0), np.full(N, -3))
    fl = (ftab, wf) if flood else None
    for c in range(2):
        qin, qsur, wd = _inputs(area0, c)
        dam = {"tab": tab, "res": res, "krls": krls, "month": 3, "begins": True, "withdrawal": wd}
        want = rt.kinematic_call(wh, wt, volr, qin, qsur, area0, p, up, 1800.0, 3, flood=fl)
        got = rt.kinematic_call(wh, wt, volr, qin, qsur, area0, p, up, 1800.0, 3, flood=fl, dam=dam)
        for g, w in zip(got, want):
            assert bits(g) == bits(w)
        assert bits(got[-4]) == bits(res) and bits(got[-3]) == bits(krls) and not got[-2].any() and bits(got[-1]) == bits(qin)
        wh, wt, volr = want[:3]
        if flood:
            fl = (ftab, want[4])


# ---- 3 and 4. closure, and the wrong variants -----------------------------------------------------------------------------------------------
def _fsum(x):
    """The exact sum of finite doubles (every one is a multiple of 2^-1074)."""
    total = 0
    for v in np.asarray(x, dtype=np.float64).tolist():
        n, d = v.as_integer_ratio()
        total += n * ((1 << 1074) // d)
    return Fraction(total, 1 << 1074)


def _closure(forest, ncall, dt=1800.0, nsub=3, variant=None):
    """ncall chained calls (months and `begins` cycling as reservoir_cases.call_time's) with the withdrawal on.  Returns (the largest
    |accumulated residual|, the sum of the calls' bounds, the largest RES - CAP over dam cells, the lowest RES - min(SMIN, first RES)
    over dam cells, the D1 cells' KRLS * C85 against the RES they met, as the largest relative difference).

    The residual of one call, in exact rational arithmetic on the doubles (D6):
        sum(WH + WT + VOLR + RES)_end - sum(WH + WT + VOLR + RES)_beg - dt (sum QIN - sum outlet QOUT) + sum RES_TAKE.

    The bound.  test_routing_kinematic_host.py counts K6's and K7's roundings of a call without dams as
        1.01 u (17 nsub SC + 5 dt Q + (nsub + 1) nsub SC + dt (SQ + SO)),   SC = S at the call's start + dt Q,
    from er dts <= VOLR and fin dts <= VUP.  A dam changes three things.  (a) The flow that leaves a dam cell is eo, and
    eo dts <= e dts + (RES - SMIN) <= VOLR + RES (a draw is limited by the storage above SMIN; a spill moves s - CAP <= RES + e dts - CAP):
    every magnitude of that count holds with RES added to S.  (b) The numbers e and eo reach K6, K5, K7 and D3 as the same doubles, so
    the roundings inside q, x and eo move no water; what rounds is s = RES + (e - eo) * dts, three roundings of magnitudes
    |e - eo| dts, |e - eo| dts and |s| <= RES + |e - eo| dts, with |e - eo| dts <= VOLR + RES: at most 4 u (VOLR + RES) + ... <=
    5 u (VOLR + RES); and the spill eo + (s - CAP) / dts, three roundings of s - CAP, the quotient and the sum, which times dts are at
    most 2 |s - CAP| + eo' dts <= 3 (VOLR + RES): together 8 u (VOLR + RES) per dam cell and sub-step, at most 8 nsub SC per call.
    (c) D2 rounds RES - t once: u RES per dam cell and call, at most u SC; RES_TAKE is t itself, and QIN enters the residual as stored.
    Hence per call, with S now sum (WH + WT + VOLR + RES),
        1.01 u (17 nsub SC + 5 dt Q + (nsub + 1) nsub SC + dt (SQ + SO) + 8 nsub SC + SC)."""
    down, up, area, p, (wh, wt, volr, wf), tab, ftab, res, krls = forest
    dams = tab["DAM"]
    res0 = res
    total, worst, bound, over, low, d1 = Fraction(0), Fraction(0), 0.0, -np.inf, np.inf, 0.0
    for c in range(ncall):
        month, begins = rc.call_time(c % 12)
        qin, qsur, wd = _inputs(area, c)
        dam = {"tab": tab, "res": res, "krls": krls, "month": month, "begins": begins, "withdrawal": wd, "variant": variant}
        wh1, wt1, v1, qout, res1, krls1, take, qin1 = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, dam=dam)
        so = _fsum(qout[down < 0])
        r = ((_fsum(wh1) + _fsum(wt1) + _fsum(v1) + _fsum(res1)) - (_fsum(wh) + _fsum(wt) + _fsum(volr) + _fsum(res))
             - Fraction(dt) * (_fsum(qin1) - so) + _fsum(take))
        total += r
        worst = max(worst, abs(total))
        q = float(np.abs(qsur).sum() + np.abs(qin1 - qsur).sum())
        sc = float(wh.sum() + wt.sum() + volr.sum() + res.sum()) + dt * q
        bound += 1.01 * U * (17 * nsub * sc + 5 * dt * q + (nsub + 1) * nsub * sc + dt * (float(np.abs(qin1).sum()) + float(so)) + 8 * nsub * sc + sc)
        over = max(over, float((res1 - tab["CAP"])[dams].max()))
        low = min(low, float((res1 - np.minimum(tab["SMIN"], res0))[dams].min()))
        on = dams & begins & (tab["MSTART"] == month)
        if on.any():
            d1 = max(d1, float(np.abs(krls1[on] * tab["C85"][on] / res[on] - 1.0).max()))
        wh, wt, volr, res, krls = wh1, wt1, v1, res1, krls1
    return float(worst), bound, over, low, d1


def test_mass_closure_in_exact_arithmetic(forest):
    """Over 50 calls on the forest the accumulated residual of D6's closure stays below the bound of _closure; no reservoir ends a call
    above CAP, none below min(SMIN, its first RES), and D1's KRLS is RES / C85 of the RES the call met, to two roundings."""
    res, bound, over, low, d1 = _closure(forest, 50)
    print(f"closure: residual {res:.3e} m3, bound {bound:.3e}; RES - CAP at most {over:.3e}; RES - min(SMIN, RES0) at least {low:.3e}; D1 {d1:.1e}")
    assert res <= bound
    assert over <= 0.0
    assert low >= 0.0
    assert d1 <= 2.0 * 2.0 * U


def test_the_wrong_variants_fail_the_same_checks(forest):
    """The statement held against wrong statements, or the inputs test nothing:
      - eo in the cell's own K6: the channel loses the regulated flow while the reservoir books the difference to the natural one;
      - a regulation after the last sub-step: RES moves once more without a flow that carries the water;
        both break the closure by orders of magnitude;
      - no spill: RES ends above CAP;  - no SMIN: a draw takes RES below min(SMIN, its first RES);
      - D1 after D2: KRLS is formed from a RES the irrigation has already drawn on."""
    own = _closure(forest, 5, variant="own_eo")
    last = _closure(forest, 5, variant="regulate_last")
    print(f"own eo: residual {own[0]:.3e} ({own[0] / own[1]:.1e} bounds); regulated last: {last[0]:.3e} ({last[0] / last[1]:.1e} bounds)")
    assert own[0] > 1.0e3 * own[1] and last[0] > 1.0e3 * last[1]
    assert _closure(forest, 5, variant="no_spill")[2] > 0.0
    assert _closure(forest, 5, variant="no_smin")[3] < 0.0
    assert _closure(forest, 5, variant="d1_after_d2")[4] > 1.0e-9


# ---- 5. physics -----------------------------------------------------------------------------------------------------------------------
def test_one_dam_through_two_years_of_a_seasonal_inflow():
    """A chain of six cells, a dam at cell 3 that holds six tenths of the year's inflow, daily calls of four sub-steps through two
    no-leap years, the month from the calendar and `begins` on its first day: RES stays within [0, CAP] and never falls below
    min(SMIN, its first RES) (no irrigation draws on it); in the second year the discharge below the dam ranges less than half as
    widely as the same cell's discharge on the same chain without the dam; KRLS is set once a year, in the month MSTART."""
    down, area, p, cap, target, beta, mstart, inflow = rc.dam_chain()
    n, d = area.size, 3
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    up = rt.upstream_map(down)
    wh = wt = volr = np.zeros(n)
    free = (wh, wt, volr)
    res, krls = 0.5 * cap, np.ones(n)
    res0 = res[d]
    qin_dam, qout_dam, sets = [], [], 0
    for day in range(730):
        doy = day % 365
        qin = np.full(n, (inflow(day) * 0.001) * area[0])
        dam = {"tab": tab, "res": res, "krls": krls, "month": rt.month_of_doy(doy), "begins": rt.month_begins(doy, doy + 1.0)}
        wh, wt, volr, qout, res1, krls1, take, _ = rt.kinematic_call(wh, wt, volr, qin, 0.5 * qin, area, p, up, 86400.0, 4, dam=dam)
        free = rt.kinematic_call(*free, qin, 0.5 * qin, area, p, up, 86400.0, 4)
        qfree, free = free[3], free[:3]
        sets += int(krls1[d] != krls[d])
        res, krls = res1, krls1
        assert 0.0 <= res[d] <= cap[d] and res[d] >= min(tab["SMIN"][d], res0) and take[d] == 0.0
        if day >= 365:
            qin_dam.append(qfree[d])
            qout_dam.append(qout[d])
    assert sets == 2
    spread_in, spread_out = max(qin_dam) - min(qin_dam), max(qout_dam) - min(qout_dam)
    print(f"without the dam {min(qin_dam):.2f} .. {max(qin_dam):.2f} m3/s, release {min(qout_dam):.2f} .. {max(qout_dam):.2f} m3/s")
    assert spread_out < 0.5 * spread_in


# ---- the input check -------------------------------------------------------------------------------------------------------------------
def _good(n):
    cap, target, beta, mstart, _, _ = rc.dam_values(n, 4)
    return cap, target, beta, mstart


@pytest.mark.parametrize("row,cell,value,text", [
    ("cap", 4, -1.0, rt.E_CAP), ("cap", 0, rc.NAN, rt.E_CAP), ("cap", 63, rc.INF, rt.E_CAP),
    ("target", 3, -1.0e-3, rt.E_TARGET), ("target", 10, rc.NAN, rt.E_TARGET), ("beta", 3, 1.5, rt.E_BETA), ("beta", 17, rc.NAN, rt.E_BETA),
    ("beta", 10, -1e-9, rt.E_BETA), ("mstart", 3, 12, rt.E_MSTART), ("mstart", 24, -1, rt.E_MSTART)])
def test_check_reservoirs_names_the_row_and_the_first_cell(row, cell, value, text):
    cap, target, beta, mstart = _good(65)
    assert cap[cell] > 0.0 or row == "cap"
    rt.check_reservoirs(cap, target, beta, mstart)
    x = {"cap": cap, "target": target[7], "beta": beta, "mstart": mstart}[row]
    x[cell] = value
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(text, cell)) + "$"):
        rt.check_reservoirs(cap, target, beta, mstart)


def test_check_reservoirs_reads_only_dam_cells_and_keeps_its_order():
    cap, target, beta, mstart = _good(65)
    assert not cap[5] > 0.0 and np.isnan(beta[5]) and mstart[5] < 0 and (target[:, 5] < 0.0).all()  # (accepted above: no dam, not read)
    beta[10], target[2, 17], cap[31] = 2.0, -1.0, -5.0
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_CAP, 31))):  # cap before every other row
        rt.check_reservoirs(cap, target, beta, mstart)
    cap[31] = 0.0
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_BETA, 10))):  # then cell by cell
        rt.check_reservoirs(cap, target, beta, mstart)
    tab = rt.reservoir_tables(*_good(65))
    assert bits(tab["SMIN"]) == bits(0.1 * tab["CAP"]) and bits(tab["C85"]) == bits(0.85 * tab["CAP"]) and not tab["BETA"][~tab["DAM"]].any()
    t = rt.reservoir_tables(np.array([5e-324]), np.zeros((12, 1)), np.ones(1), np.zeros(1, np.int32))
    assert t["DAM"][0] and t["SMIN"][0] == 0.0 and t["C85"][0] == 5e-324  # (0.1 of the smallest double rounds to zero, 0.85 of it to itself)


def _build_checks(tmp_path, flags, name):
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "c", "reservoir_checks.cc")
    inc = os.path.join(ROOT, "elmkernels_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan-ubsan"])
def test_the_host_check_as_a_program(tmp_path, flags):
    """tests/c/reservoir_checks.cc drives elmk_maps.h: reservoir_check and the calendar: every refusal with the text and the cell
    check_reservoirs gives, the tables bit for bit reservoir_tables', padding cells zero, every doy's month month_of_doy's."""
    exe = _build_checks(tmp_path, flags, "reservoir_checks")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    lines = dict(s.split(": ", 1) for s in out)
    assert lines["ncells 0"] == rt.E_NCELLS and lines["null cap"] == "null argument" and lines["null mstart"] == "null argument"
    n = 5
    cap = np.array([0.0, 2.0e9, 5e-324, 7.5e8, 0.0])
    for name, text in lines.items():
        m = re.fullmatch(r"bad (\w+) (\d)", name)
        if m:
            want = {"CAP": rt.E_CAP, "TARGET": rt.E_TARGET, "BETA": rt.E_BETA, "MSTART": rt.E_MSTART}[m.group(1)]
            assert text == rt.e_cell(want, int(m.group(2))), name
    assert sum(name.startswith("bad ") for name in lines) >= 12
    assert lines["no dam holds anything"] == "ok" and lines["cap before the rest"] == rt.e_cell(rt.E_CAP, 4)
    vals = lines["valid"].split()
    assert vals[0] == "ok"
    got = np.array([float.fromhex(v) for v in vals[1:1 + 16 * n]]).reshape(16, n)
    ms = np.array([int(v) for v in vals[1 + 16 * n:]])
    target = np.array([[10.0 * (m + 1) + c for c in range(n)] for m in range(12)])
    tab = rt.reservoir_tables(cap, target, np.array([9.0, 0.25, 1.0, 0.0, -1.0]), np.array([40, 11, 0, 5, -2]))
    want = np.concatenate([np.stack([tab["CAP"], tab["SMIN"], tab["C85"], tab["BETA"]]), tab["TARGET"]])
    assert bits(got) == bits(want) and (ms == tab["MSTART"]).all()
    assert lines["sixty-five cells"] == "ok"
    months = [int(v) for v in lines["months"].split()]
    assert months == [rt.month_of_doy(d) for d in range(-1, 366)]
    begins = [int(v) for v in lines["begins"].split()]
    assert begins == list(rt.MONTH_FIRST_DOY) and lines["begins off the hour"] == "0"


# ---- Hanasaki's rules, the calendar ------------------------------------------------------------------------------------------------------
def test_reservoir_targets_follow_hanasaki():
    inflow = np.array([5.0, 9.0, 20.0, 40.0, 60.0, 45.0, 30.0, 18.0, 10.0, 6.0, 4.0, 3.0])
    im = inflow.mean()
    year = im * 365.0 * 86400.0
    none = np.zeros(12)
    t, b, m = rt.reservoir_targets(inflow, none, np.array([0.1 * year, 0.5 * year, 2.0 * year]))
    assert np.allclose(t, im) and np.allclose(b, [0.04, 1.0, 1.0]) and (m == 7).all()  # the inflow falls below its mean in August
    demand = np.array([0, 0, 0, 2.0, 6.0, 10.0, 10.0, 6.0, 2.0, 0, 0, 0]) * 6.0  # dm = 18 >= im / 2
    t, _, _ = rt.reservoir_targets(inflow, demand, 0.5 * year)
    assert np.allclose(t[:, 0], (im / 2.0) * (1.0 + demand / demand.mean())) and np.isclose(t.mean(), im)
    small = demand / 6.0  # dm = 3 < im / 2
    t, _, _ = rt.reservoir_targets(inflow, small, 0.5 * year)
    assert np.allclose(t[:, 0], im + small - small.mean()) and (t >= 0.0).all()
    rt.check_reservoirs(np.full(1, 0.5 * year), t, np.ones(1), np.zeros(1, np.int32))


def test_the_calendar():
    assert [rt.month_of_doy(d) for d in rt.MONTH_FIRST_DOY] == list(range(12)) and rt.month_of_doy(364) == 11 and rt.month_of_doy(365) == 0
    assert [rt.month_of_doy(d - 1) for d in rt.MONTH_FIRST_DOY[1:]] == list(range(11)) and rt.month_of_doy(58) == 1 and rt.month_of_doy(59) == 2
    assert all(rt.month_begins(d, d + 1.0) for d in rt.MONTH_FIRST_DOY)
    assert not rt.month_begins(31, 32.0 + 1800.0 / 86400.0) and not rt.month_begins(30, 31.0) and not rt.month_begins(365, 366.0)


# ---- the header and the bindings -----------------------------------------------------------------------------------------------------------
def test_the_header_the_bindings_and_the_constants_agree():
    text = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert "enum { ELMK_ROUTE_RES = 10, ELMK_ROUTE_KRLS = 11, ELMK_ROUTE_RES_TAKE = 12 };" in text
    assert (rt.RES, rt.KRLS, rt.RES_TAKE) == (st.ROUTE_RES, st.ROUTE_KRLS, st.ROUTE_RES_TAKE) == (10, 11, 12)
    for name in ("enable", "init", "time", "budget", "clear"):
        assert f"int elmk_routing_reservoir_{name}(elmk_ctx *ctx" in text and f"elmk_routing_reservoir_{name}" in L.SIGNATURES
    for k in range(9):
        assert f" * D{k}. " in text
    maps = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    for msg in (rt.E_CAP, rt.E_TARGET, rt.E_BETA, rt.E_MSTART):
        assert f'"{msg}"' in maps
