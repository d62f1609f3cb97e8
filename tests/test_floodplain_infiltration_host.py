"""Floodplain infiltration without a GPU (include/elmk.h "floodplain infiltration"): the river's budget F6 and the budget of land and
river together in exact rational arithmetic against bounds counted from the statement's roundings, the soil under a flood with and
without the extension, the guard of F1 on every edge value, the bits of the plain stages where no cell is flooded, the census the
device test relies on, the host check of elmkernels_amd/csrc/elmk_maps.h through a stand-alone program (plain and under the address and
undefined-behaviour sanitizers), and the header's constants and the bindings."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics
from elmkernels_amd import hydrology as hy
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import floodplain_infiltration_cases as fc
from tests.support import ROOT, bits

U = 2.0 ** -53  # the unit roundoff of fp64
NAN, INF = float("nan"), float("inf")
F = Fraction
DT, NSUB = fc.DT, 4


def _fsum(x):
    """The exact sum of finite doubles."""
    return sum((F(v) for v in np.asarray(x, dtype=np.float64).reshape(-1).tolist()), F(0))


def _abs(x):
    return float(np.abs(np.asarray(x, dtype=np.float64)).sum())


# ---- the storm on the chain ---------------------------------------------------------------------------------------------------------------
def _river_residual(before, after, qland, down, dt, nsub):
    """F6 over one call in exact arithmetic, and its bound.  before, after: the river's rows (host_step's dicts).  The bound is I7's
    (tests/test_routing_inundation_host.py: (19 + nsub + 1) nsub SC + 5 dt Q + dt (SQ + SO), SC the storages at the call's start plus dt Q)
    over the storages F5 leaves, plus F5's two roundings per cell, fl(QLAND dt) and fl(WF - .), each at most u times what it rounds:
    u (|WF| + 2 dt |QLAND|)."""
    qin, qout = after["qin"], after["qout"]
    so = _fsum(qout[down < 0])
    stores = lambda r: sum(_fsum(r[k]) for k in ("wh", "wt", "volr", "wf"))  # noqa: E731
    res = stores(after) - stores(before) - F(dt) * (_fsum(qin) - so - _fsum(qland))
    q = 2.0 * _abs(qin)
    sc = sum(_abs(before[k]) for k in ("wh", "wt", "volr", "wf")) + dt * (q + _abs(qland))
    bound = 1.01 * U * ((19 + (nsub + 1)) * nsub * sc + 5 * dt * q + dt * (_abs(qin) + float(so)) + _abs(before["wf"]) + 2.0 * dt * _abs(qland))
    return abs(res), bound


def _flooded_start(G):
    """The chain's rivers a fifth over their banks with 3e6 m3 on every floodplain, brought to one level by a call without input."""
    tab = rt.inundation_tables(G["area"], G["p"], G["rdepth"], G["eprof"])
    G = dict(G, volr=tab["VC"] * 1.2, wf=np.full(G["ncells"], 3.0e6))
    return G, fc.river0(G, nsub=NSUB)


def _chain(G, f, rows, river, nsteps, on, rain):
    """nsteps host steps; per step (fields, rows, fpi, wb, river before, river after, qland)."""
    out = []
    for s in range(nsteps):
        f = fc.set_rain(f, rain if s < 2 else 0.0)
        f, wb = fc.begin(f, rows)
        before = river
        f, rows, _, fpi, wb, river, qland = fc.host_step(f, rows, wb, river, G, nsub=NSUB, on=on)
        out.append((f, rows, fpi, wb, before, river, qland))
    return out


def test_the_rivers_budget_closes_with_qland():
    """F6 over five chained calls on the storm chain: the change of sum WH + sum WT + sum VOLR + sum WF over a call is
    dt (sum QIN - sum outlet QOUT - sum QLAND) inside the counted bound, in every call; without QLAND in it the identity misses the bound
    by orders of magnitude; WF falls by what the land took."""
    G, f = fc.storm_case()
    G, river = _flooded_start(G)
    steps = _chain(G, f, G["rows"], river, fc.NSTEPS, True, 40.0 / 3600.0)
    total = 0.0
    for s, (_, _, fpi, _, before, after, qland) in enumerate(steps):
        res, bound = _river_residual(before, after, qland, G["down"], DT, NSUB)
        print(f"call {s}: residual {float(res):.3e} m3, bound {bound:.3e} m3, sum QLAND dt {float(_fsum(qland)) * DT:.3e} m3")
        assert res <= bound, (s, float(res), bound)
        assert (qland > 0.0).all() and (fpi[hy.FPI_QFLX_DRAIN] > 0.0).all() and (fpi[hy.FPI_FRAC] > 0.0).all()
        without, _ = _river_residual(before, after, np.zeros_like(qland), G["down"], DT, NSUB)
        assert without > 1.0e6 * bound
        total += float(_fsum(qland)) * DT
    assert total > 1.0e5  # m3
    assert bits(rt.land_budget(steps[-1][6])) == bits(np.array([diagnostics.reduce_min_max_sum(steps[-1][6])[2]]))


def test_land_and_river_close_together():
    """On a map whose weights sum to 1 per cell, per step: the area-weighted sum of ENDWB - BEGWB (as volume) plus the change of the
    river's stores equals the external terms alone - rain less evaporation over the columns, less the outlet's discharge - and the
    columns' own ERRH2O, which is the budget error of the soil hydrology by itself and of rounding size (held under 1e-9 mm here): sum
    QLAND dt cancels against the columns' d, and sum QIN dt against their QRUNOFF.  The bound counts, per column, W4's eight roundings
    (each at most u times the larger of the two water masses and of the step's fluxes, as volume through w area / 1000); per cell, R1's
    and F5's aggregates ((terms + 2) roundings each, u times the sum of the terms' magnitudes, times dt); and the river's bound above.
    With the extension off the same chain leaves the soil under the flood at the dry chain's water: the gap the extension closes."""
    G0, f0 = fc.storm_case()
    G, river = _flooded_start(G0)
    ptr, col, w = G["map"]
    area_of = np.repeat(G["area"], np.diff(ptr))  # per term
    vol = lambda x: x[col] * w * 0.001 * area_of  # noqa: E731  (mm over a column -> m3 of its cell, per term)
    volx = lambda x: sum((F(a) * F(b) * F(c) / 1000 for a, b, c in zip(x[col].tolist(), w.tolist(), area_of.tolist())), F(0))  # noqa: E731
    nterm = int(np.diff(ptr).max())
    steps = _chain(G, f0, G["rows"], river, fc.NSTEPS, True, 40.0 / 3600.0)
    for s, (f, rows, fpi, wb, before, after, qland) in enumerate(steps):
        d, q = fpi[hy.FPI_QFLX_DRAIN], wb[hy.WB_QRUNOFF]
        land = volx(wb[hy.WB_ENDWB]) - volx(wb[hy.WB_BEGWB])
        stores = lambda r: sum(_fsum(r[k]) for k in ("wh", "wt", "volr", "wf"))  # noqa: E731
        outlet = _fsum(after["qout"][G["down"] < 0])
        external = F(DT) * (volx(f["forc_rain"]) - volx(f["qflx_evap_tot"])) - F(DT) * outlet
        res = abs(land + (stores(after) - stores(before)) - external - volx(wb[hy.WB_ERRH2O]))
        m = np.maximum(np.abs(wb[hy.WB_ENDWB]) + np.abs(wb[hy.WB_BEGWB]), DT * (np.abs(f["forc_rain"]) + np.abs(d) + np.abs(q) + np.abs(f["qflx_evap_tot"])))
        b_w4 = 1.01 * U * 8.0 * float(np.abs(vol(m)).sum())
        b_agg = 1.01 * U * (nterm + 2) * DT * float(np.abs(vol(q)).sum() + np.abs(vol(d)).sum())
        b_river = _river_residual(before, after, qland, G["down"], DT, NSUB)[1]
        bound = b_w4 + b_agg + b_river
        print(f"step {s}: residual {float(res):.3e} m3, bound {bound:.3e} (W4 {b_w4:.2e}, aggregates {b_agg:.2e}, river {b_river:.2e}); "
              f"largest |ERRH2O| {np.abs(wb[hy.WB_ERRH2O]).max():.2e} mm; land took {float(volx(d)) * DT:.3e} m3")
        assert res <= bound, (s, float(res), bound)
        assert np.abs(wb[hy.WB_ERRH2O]).max() < 1.0e-9
        # the two exchanges themselves are far above the bound: they cancel, they are not small
        assert float(volx(d)) * DT > 1.0e6 * bound
    # the regression: with the extension off the columns do not see the flood
    off = _chain(G, f0, G["rows"], river, fc.NSTEPS, False, 40.0 / 3600.0)
    dry_G = dict(G0)
    dry = _chain(dry_G, f0, G0["rows"], fc.river0(G0, spin=False), fc.NSTEPS, False, 40.0 / 3600.0)
    assert (off[-1][5]["wf"] > 0.0).all()  # (half under water)
    for k in ("h2osoi_liq", "h2osfc"):
        assert bits(off[-1][0][k]) == bits(dry[-1][0][k]), k
    assert bits(off[-1][3][hy.WB_ENDWB]) == bits(dry[-1][3][hy.WB_ENDWB])
    assert (steps[-1][3][hy.WB_ENDWB] > off[-1][3][hy.WB_ENDWB] + 1.0).all()  # every wetted column holds over a millimetre more
    assert (steps[-1][5]["wf"] < off[-1][5]["wf"]).all()


# ---- the guard --------------------------------------------------------------------------------------------------------------------------
def _loam_fields(n, seed=3):
    G, f = fc.storm_case(ncol_per_cell=1)
    assert G["ncols"] == 8
    idx = np.arange(n) % 8
    f = {k: np.ascontiguousarray(np.asarray(v)[idx]) for k, v in f.items()}
    return fc.set_rain(f, 1.0e-4), np.ascontiguousarray(G["rows"][:, idx])


def test_the_guard_keeps_the_drain_from_going_negative_or_nan():
    """Every column in a cell of its own: WF zero, negative zero, negative, denormal, NaN, +inf, -inf and 1e300; FLOOD_FRAC zero,
    negative and NaN; area zero, negative and NaN; a column in no cell; a NaN qinmax over finite and infinite water.  d is never
    negative, and over an area the routing accepts (finite) never NaN: a NaN a loses the comparison and d = b."""
    wf = [0.0, -0.0, -3.5e4, 5e-324, NAN, INF, -INF, 1e300, 2.0e6, 2.0e6, 2.0e6, 2.0e6, 2.0e6, 2.0e6, 2.0e6, 2.0e6, INF, 10.0]
    ff = [0.5] * 8 + [0.0, -0.1, NAN, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    ar = [1.0e8] * 11 + [0.0, -1.0e8, NAN, 1.0e8, 1.0e8, 1.0e8, 1.0e8]
    n = len(wf)
    f, rows = _loam_fields(n)
    cell = np.arange(n, dtype=np.int32)
    cell[14] = -1
    rows[hy.WTFACT, 15:17] = NAN  # qinmax NaN (fsat is)
    passes = [3, 5, 7, 15, 16, 17]
    res = hy.step({k: f[k] for k in fc.STEP_FIELDS}, rows, DT, rof=(cell, np.array(wf), np.array(ff), np.array(ar)))
    plain = hy.step({k: f[k] for k in fc.STEP_FIELDS}, rows, DT)
    fpi = res[2]
    d, hr, fr = fpi[hy.FPI_QFLX_DRAIN], fpi[hy.FPI_H2OROF], fpi[hy.FPI_FRAC]
    assert not (d < 0.0).any() and not np.isnan(d).any() and not np.signbit(d).any()
    for c in range(n):
        if c in passes:
            assert fr[c] == 0.5 and hr[c] == (wf[c] / ar[c]) * 1000.0, c
        else:
            assert bits(fpi[:, c]) == bits(np.zeros(3)), c
            for k in ("h2osoi_liq", "h2osfc"):  # ... and every other output keeps the bits of the plain stage
                assert bits(res[0][k][c]) == bits(plain[0][k][c]), (c, k)
            assert bits(res[1][:, c]) == bits(plain[1][:, c]), c
    assert hr[3] == 0.0 and d[3] == 0.0 and fr[3] == 0.5  # the denormal passes the guard and underflows to no water: b = 0, the smaller
    for c in (5, 7):  # WF = +inf, and 1e300: d = a = FLOOD_FRAC qinmax, and qinmax is at most the top three layers' smallest HKSAT
        assert hr[c] == (INF if c == 5 else 1e300 / 1.0e8 * 1000.0) and 0.0 < d[c] <= 0.5 * rows[hy.HKSAT:hy.HKSAT + 3, c].min(), c
    assert d[15] == hr[15] / DT and np.isnan(res[1][hy.FSAT, 15])  # NaN qinmax: a < b is false, d = b
    assert d[16] == INF  # ... over infinite water too
    assert d[17] == hr[17] / DT == (10.0 / 1.0e8 * 1000.0) / DT  # a >= b
    assert (res[1][hy.QFLX_INFL][[5, 7, 17]] > plain[1][hy.QFLX_INFL][[5, 7, 17]]).all()  # F2: QFLX_INFL carries the term
    # both infinite, area and water, is the one way to a NaN b - and the routing refuses such an area
    far = hy.step({k: f[k][:1] for k in fc.STEP_FIELDS}, rows[:, :1], DT, rof=(np.zeros(1, np.int32), np.array([INF]), np.array([0.5]), np.array([INF])))
    assert np.isnan(far[2][hy.FPI_QFLX_DRAIN, 0])
    with pytest.raises(ValueError, match=re.escape(rt.E_AREA)):
        rt.check_network(np.array([-1], np.int32), np.array([1.0e3]), np.array([INF]))


def test_no_flooded_cell_keeps_the_bits_of_the_plain_stages():
    """A context in which no cell is flooded: step, water_balance_end and kinematic_call with the arguments give the bits of the calls
    without them on every existing row, column and cell; the new rows are zero."""
    G = fc.case("wide", 31)
    G["wf"] = np.zeros(G["ncells"])
    G["rdepth"] = np.full(G["ncells"], 1.0e6)  # banks that no river of the case climbs
    f, rows = fc.host_fields(G["cols"]), G["rows"]
    river_on = river_off = fc.river0(G)
    assert not river_on["wf"].any() and not river_on["frac"].any()
    for s in range(2):
        f1, wb1 = fc.begin(f, rows)
        a = fc.host_step(f1, rows, wb1, river_on, G, on=True)
        b = fc.host_step(f1, rows, wb1, river_off, G, on=False)
        assert not a[3].any() and not np.signbit(a[3]).any() and not a[6].any()
        for k in hy.WRITES:
            assert bits(a[0][k]) == bits(b[0][k]), (s, k)
        assert bits(a[1]) == bits(b[1]) and bits(a[4]) == bits(b[4])
        for k in ("wh", "wt", "volr", "qout", "wf", "depth", "frac", "qin"):
            assert bits(a[5][k]) == bits(b[5][k]), (s, k)
        f, rows, river_on, river_off = a[0], a[1], a[5], b[5]
    assert np.isnan(a[1][hy.QFLX_SURF]).any()  # (the NaN column is among them)


def test_the_wide_shape_holds_every_branch_in_every_step():
    """The census the device test relies on, on the host chain of the same inputs: in the wide shape every branch of F1 is taken in
    every step, the column with the NaN qinmax drains b, and the shapes are what their names say."""
    G = fc.case("wide", 31)
    ptr, col, w = G["map"]
    cnt = np.diff(ptr)
    assert G["ncols"] == 5003 and G["ncells"] == 70 and cnt[fc.BIG_CELL] == 2100 and not cnt[[0] + list(range(60, 68))].any()
    assert (G["cellof"] < 0).sum() == 300 and (cnt[np.setdiff1d(np.arange(70), [0] + list(range(60, 68)))] >= 1).all()
    assert np.unique(col).size == col.size and (w > 0.0).all() and np.add.reduceat(w, ptr[:-1][cnt > 0]).max() <= 1.0 + 1e-12
    n1, c1, p1, col1, _ = fc.cell_map("single")
    assert (n1, c1) == (1010, 1001) and (np.diff(p1) == 1).all() and fc.cell_map("one")[:2] == (1, 1)
    f, rows, river = fc.host_fields(G["cols"]), G["rows"], fc.river0(G)
    for s in range(fc.NSTEPS):
        f, wb = fc.begin(f, rows)
        before = river
        f, rows, _, fpi, wb, river, qland = fc.host_step(f, rows, wb, river, G)
        took = np.bincount(fc.census(G["cellof"], before["wf"], before["frac"], fpi), minlength=len(fc.BRANCHES))
        assert (took > 0).all(), (s, dict(zip(fc.BRANCHES, took.tolist())))
        q = G["nanq"]
        assert fpi[hy.FPI_QFLX_DRAIN, q] == fpi[hy.FPI_H2OROF, q] / DT > 0.0 and np.isnan(rows[hy.FSAT, q])
        assert not (fpi[hy.FPI_QFLX_DRAIN] < 0.0).any() and not np.isnan(fpi[hy.FPI_QFLX_DRAIN]).any()
        edge = before["wf"][2:18:2]
        assert np.isnan(edge).any() and (edge < 0.0).any()  # the edge values of WF are still in their cells


# ---- F0: the restatement, and the same check in C: tests/c/floodplain_infiltration_checks.cc -----------------------------------------------
def test_cellof_names_the_cell_of_every_column():
    assert fc.cellof(5, np.array([0, 2, 2, 5]), np.array([3, 0, 4, 1, 2])).tolist() == [0, 2, 2, 0, 2]
    assert fc.cellof(9, np.array([0, 1, 2]), np.array([8, 0])).tolist() == [1, -1, -1, -1, -1, -1, -1, -1, 0]
    with pytest.raises(ValueError, match="column 2 is in more than one cell"):
        fc.cellof(6, np.array([0, 3, 6]), np.array([5, 2, 3, 2, 5, 3]))


def _say(ncols, ptr, col, show=True):
    try:
        g = fc.cellof(ncols, np.array(ptr, np.int64), np.array(col, np.int64))
    except ValueError as e:
        return re.search(r"column (\d+) ", str(e)).group(1)
    except IndexError:
        return "-2"
    if show:
        return " ".join(["-1"] + [str(v) for v in g.tolist()])
    return f"-1 size={g.size} sum={int(g.astype(np.int64).sum())} none={int((g < 0).sum())}"


def expected():
    big = list(range(99999, -1, -1))
    ptr = [100 * r for r in range(1001)]
    return [("one column in one cell", _say(1, [0, 1], [0])), ("one cell without terms", _say(3, [0, 0], [])),
            ("every column once", _say(5, [0, 2, 2, 5], [3, 0, 4, 1, 2])), ("columns in no cell", _say(9, [0, 1, 2], [8, 0])),
            ("empty cells around a full one", _say(4, [0, 0, 0, 3, 3], [2, 0, 3])), ("last column twice", "4"), ("twice in one cell", "0"),
            ("two repeats, the first in term order wins", "2"), ("column out of range before a repeat", "-2"),
            ("column negative before a repeat", "-2"), ("repeat before a column out of range", "0"), ("no columns at all", "-1"),
            ("100000 columns over 1000 cells", _say(100000, ptr, big, False)), ("... under 100003 columns", _say(100003, ptr, big, False)),
            ("... and one again", "77")]


def _build_and_run(tmp, sanitized):
    exe = str(tmp / ("floodplain_infiltration_checks_san" if sanitized else "floodplain_infiltration_checks"))
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "floodplain_infiltration_checks.cc"), "-o", exe]
    if sanitized:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return None, r.stderr.decode()
    # stand-alone: the program has its own main and nothing of it is loaded into Python.  (Leak detection needs ptrace, which a
    # container may deny.)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()
    return [tuple(s.split(": ", 1)) for s in r.stdout.decode().splitlines()], ""


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("floodplain_infiltration_checks")


def test_every_case_returns_the_first_shared_column_or_the_cells(tmp):
    lines, err = _build_and_run(tmp, False)
    assert lines is not None, err
    want = expected()
    assert [g[0] for g in lines] == [w[0] for w in want]
    for g, w in zip(lines, want):
        assert g == w, g[0]
    assert lines[2][1] == "-1 0 2 2 0 2" and lines[12][1].startswith("-1 size=100000 sum=") and lines[13][1].endswith("none=3")


def test_the_same_program_under_the_sanitizers(tmp):
    """-fsanitize=address,undefined, run stand-alone: an out-of-range read of the map or write of cellof ends the program."""
    lines, err = _build_and_run(tmp, True)
    if lines is None:
        pytest.fail("the host compiler does not link the sanitizers' static runtimes here:\n" + err[-400:])
    assert lines == expected()


def test_the_cost_tool_imports_without_device_or_library(tmp_path):
    """tests/tools/cost_floodplain_infiltration.py imports without a device and without the built library, as
    tests/test_cost_tools_host.py asks of the *_cost.py tools, and takes its protocol from costlib."""
    import sys

    tools = os.path.join(ROOT, "tests", "tools")
    src = open(os.path.join(tools, "cost_floodplain_infiltration.py")).read()
    assert "import costlib as CL" in src and "perf_counter" not in src
    code = ("import sys, importlib\nsys.path.insert(0, sys.argv[1])\nm = importlib.import_module('cost_floodplain_infiltration')\n"
            "print('imported', m.CALLS == m.CR.CALLS, m.TIERS)\n")
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, tools], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "imported True ('none', 'tenth', 'all')", r.stderr[-2000:]


# ---- the header and the bindings ------------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("enable", "read", "budget", "clear")


def test_header_constants_and_bindings():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert h.index("/* ---- stream temperature ----") < h.index("/* ---- floodplain infiltration ----") < h.index("/* ---- feature rows")
    assert "enum { ELMK_FPI_H2OROF = 0, ELMK_FPI_FRAC = 1, ELMK_FPI_QFLX_DRAIN = 2, ELMK_FPI_NROWS = 3 };" in h
    assert "enum { ELMK_ROUTE_QLAND = 20 };" in h and "enum { ELMK_ROWS_FLOODPLAIN = 7 };" in h
    assert (hy.FPI_H2OROF, hy.FPI_FRAC, hy.FPI_QFLX_DRAIN) == (st.FPI_H2OROF, st.FPI_FRAC, st.FPI_QFLX_DRAIN) == (0, 1, 2)
    assert rt.QLAND == st.ROUTE_QLAND == 20 and st.ROWS_FLOODPLAIN == 7
    for name in ENTRY_POINTS:
        assert re.search(rf"^int elmk_floodplain_infiltration_{name}\(", h, re.M) and f"elmk_floodplain_infiltration_{name}" in L.SIGNATURES, name
        assert hasattr(st.ELMState, "floodplain_infiltration_" + name)
    for k in range(9):
        assert f" F{k} " in h
    hpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    for name in ENTRY_POINTS:
        assert f"elmk_floodplain_infiltration_{name}(" in hpp, name
    # the kernels: template forms of the existing ones, no hint and no fence
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_routing.hip")).read()
    assert "template <bool WITHDRAW, bool DAM = false, bool HEAT = false, bool LAND = false>\n__global__ __launch_bounds__(256) void k_kinematic_prep(" in k
    assert "nontemporal_" not in k and "__threadfence" not in k
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_soil_hydrology.hip")).read()
    assert "template <bool FROST, bool ROF>\n__global__ __launch_bounds__(256) void k_soil_hydrology(" in k
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_water_balance.hip")).read()
    assert "template <bool FROST, bool IRRIG, bool LAND, class... Q>" in k
