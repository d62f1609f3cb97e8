"""Hillslope lateral flow without a GPU (include/elmk.h "hillslope lateral flow"): every refusal of hillslope_check with its text, on
the host restatement and through a stand-alone program over elmkernels_amd/csrc/elmk_maps.h (plain and under the address and
undefined-behaviour sanitizers); the uphill map for in-degrees 0 to 8; the three consequences of the statement; the census the device
test relies on; the two budgets in exact rational arithmetic against counted bounds; the physical check; the header's constants and the
bindings."""
import os
import re
import subprocess
from fractions import Fraction as F

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics
from elmkernels_amd import hydrology as hy
from elmkernels_amd import state as st
from tests import hillslope_cases as hc
from tests.hydrology_cases import water_mass
from tests.support import ROOT, bits

NAN, INF = float("nan"), float("inf")
U, DT = hc.U, hc.DT


def _fsum(x):
    return sum((F(v) for v in np.asarray(x, dtype=np.float64).reshape(-1).tolist()), F(0))


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
def _set(down, **kw):
    n = len(down)
    s = dict(down=np.array(down, np.int32), dist=np.full(n, 50.0), width=np.full(n, 30.0), area=np.full(n, 1500.0), elev=np.full(n, 2.0), k=10.0)
    for k, v in kw.items():
        if k == "k":
            s["k"] = v
        else:
            row, col = k.split("_")
            s[row][int(col)] = v
    return s


def _say(s, show=True, null_elev=False):
    text, col = hy.hillslope_check(s["down"], s["dist"], s["width"], s["area"], None if null_elev else s["elev"], s["k"])
    if text is not None:
        return f"{text} @{col}"
    up = hy.hillslope_map(s["down"])
    nup = int((up >= 0).sum(axis=0).max())
    if show:
        return f"ok nup={nup} up=" + "|".join(" ".join(str(v) for v in row) for row in up.tolist())
    return f"ok nup={nup} up=size={up.size} sum={int(up.astype(np.int64).sum())} none={int((up < 0).sum())}"


def cases():
    out = [("one column to the stream", _set([-1])), ("one column on no hillslope", _set([-2])), ("a chain of five", _set([-1, 0, 1, 2, 3]))]
    out += [(f"in-degree {k}", _set([-1] + [0] * k + [-2])) for k in range(9)]
    out += [("slots ascend whatever the order", _set([3, 3, -1, 2, 3, 2])), ("null argument", None), ("down below -2", _set([-1, -3, 0])),
            ("down past the columns", _set([-1, 3, 0])), ("self-loop", _set([-1, 0, 2])), ("range before self-loop", _set([0, 9])),
            ("into a column on no hillslope", _set([-2, 0, -1])), ("self-loop before a -2 target", _set([-2, 0, 2])),
            ("nine uphill columns", _set([-1] + [0] * 9)), ("a cycle of two", _set([-1, 2, 1])), ("a cycle behind a tail", _set([1, 2, 3, 1, -1])),
            ("in-degree before a cycle", _set([1] + [0] * 10))]
    d = [-1, 0, -2]
    off = dict(dist_2=NAN, width_2=0.0, area_2=-INF, elev_2=NAN, elev_0=-3.0)
    out += [("dist before width", _set(d, dist_1=0.0, width_0=NAN)), ("width NaN", _set(d, width_0=NAN)), ("area negative", _set(d, area_1=-1.0)),
            ("area infinite", _set(d, area_1=INF)), ("elev infinite", _set(d, elev_0=INF)),
            ("nothing is asked of a column on no hillslope", _set(d, **off)), ("k_aniso zero", _set(d, k=0.0, **off)),
            ("k_aniso NaN", _set(d, k=NAN, **off)), ("k_aniso infinite", _set(d, k=INF, **off))]
    long = np.arange(200000) - 1
    out.append(("a chain of 200000", _set(long)))
    long = long.copy()
    long[0] = long.size - 1
    out.append(("... closed into a cycle", _set(long)))
    return out


def expected():
    out = []
    for name, s in cases():
        if s is None:
            out.append((name, _say(_set([-1]), null_elev=True)))
        else:
            out.append((name, _say(s, show=len(s["down"]) < 100)))
    return out


REFUSALS = {"null argument": "null argument @-1", "down below -2": "down outside {-2, -1} and [0, ncols) @1",
            "down past the columns": "down outside {-2, -1} and [0, ncols) @1", "self-loop": "down equals its own index @2",
            "range before self-loop": "down outside {-2, -1} and [0, ncols) @1",
            "into a column on no hillslope": "down names a column on no hillslope @1", "self-loop before a -2 target": "down equals its own index @2",
            "nine uphill columns": "more than 8 uphill columns drain into one column @9", "a cycle of two": "the hillslope has a cycle @1",
            "a cycle behind a tail": "the hillslope has a cycle @0", "in-degree before a cycle": "more than 8 uphill columns drain into one column @9",
            "dist before width": "dist not finite and > 0 @1", "width NaN": "width not finite and > 0 @0", "area negative": "area not finite and > 0 @1",
            "area infinite": "area not finite and > 0 @1", "elev infinite": "elev not finite @0", "k_aniso zero": "k_aniso not finite and > 0 @-1",
            "k_aniso NaN": "k_aniso not finite and > 0 @-1", "k_aniso infinite": "k_aniso not finite and > 0 @-1",
            "... closed into a cycle": "the hillslope has a cycle @0"}


def test_every_refusal_has_its_text_and_its_column():
    got = dict(expected())
    for name, want in REFUSALS.items():
        assert got[name] == want, name
    assert {k for k, v in got.items() if not v.startswith("ok ")} == set(REFUSALS)
    assert got["nothing is asked of a column on no hillslope"] == "ok nup=1 up=1 -1 -1"
    assert hy.hillslope_check(np.zeros(0, np.int32), [], [], [], [], 1.0) == ("ncols outside 1 .. 2^31-1", -1)


def test_the_map_for_in_degrees_0_to_8():
    got = dict(expected())
    for k in range(9):
        up = hy.hillslope_map([-1] + [0] * k + [-2])
        npad = 1 if k <= 1 else 2 if k <= 2 else 4 if k <= 4 else 8
        assert up.shape == (npad, k + 2) and up.dtype == np.int32
        assert up[:, 0].tolist() == list(range(1, k + 1)) + [-1] * (npad - k) and (up[:, 1:] == -1).all()
        assert got[f"in-degree {k}"].startswith(f"ok nup={k} up=")
    assert got["slots ascend whatever the order"] == "ok nup=3 up=-1 -1 3 0 -1 -1|-1 -1 5 1 -1 -1|-1 -1 -1 4 -1 -1|-1 -1 -1 -1 -1 -1"
    up = hy.hillslope_map([3, 3, -1, 2, 3, 2])
    assert up.shape == (4, 6) and up[:, 3].tolist() == [0, 1, 4, -1] and up[:, 2].tolist() == [3, 5, -1, -1]
    assert got["a chain of 200000"] == f"ok nup=1 up=size=200000 sum={sum(range(1, 200000)) - 1} none=1"


def _build_and_run(tmp, sanitized):
    exe = str(tmp / ("hillslope_checks_san" if sanitized else "hillslope_checks"))
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "hillslope_checks.cc"), "-o", exe]
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
    return tmp_path_factory.mktemp("hillslope_checks")


def test_the_c_check_says_what_the_restatement_says(tmp):
    lines, err = _build_and_run(tmp, False)
    assert lines is not None, err
    want = expected()
    assert [g[0] for g in lines] == [w[0] for w in want]
    for g, w in zip(lines, want):
        assert g == w, g[0]


def test_the_same_program_under_the_sanitizers(tmp):
    """-fsanitize=address,undefined, run stand-alone: an out-of-range read of down or write of the map ends the program."""
    lines, err = _build_and_run(tmp, True)
    if lines is None:
        pytest.fail("the host compiler does not link the sanitizers' static runtimes here:\n" + err[-400:])
    assert lines == expected()


def test_every_shape_is_accepted():
    for name in hc.SHAPES:
        G = hc.shape(name)
        assert hy.hillslope_check(*hc.lat_of(G)) == (None, -1), name
    assert hy.hillslope_map(hc.shape("one")["down"]).shape[0] == 1 and hy.hillslope_map(hc.shape("chain5")["down"]).shape[0] == 1
    for k in (1, 2, 4, 8):
        assert hy.hillslope_map(hc.shape(f"star{k}")["down"]).shape[0] == k
    G = hc.shape("wide")
    assert G["ncols"] == 1001 and (G["down"] == -2).sum() > 100 and hy.hillslope_map(G["down"]).shape[0] == 8
    assert G["down"][255] == 256  # a neighbour across the workgroup boundary


# ---- the three consequences ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide():
    G = hc.shape("wide")
    cols, scal, soil, rows = hc.columns(G, 21)
    return G, cols, rows, hc.host_chain(G, cols, rows, 6)


def test_all_off_hillslope_keeps_the_bits_of_the_plain_stage(wide):
    G, cols, rows, _ = wide
    off = dict(G, down=np.full(G["ncols"], -2, np.int32))
    a = hc.host_chain(off, cols, rows, 2)
    b = hc.host_chain(G, cols, rows, 2, on=False)
    for (fa, ra, hs, _), (fb, rb, _, _) in zip(a, b):
        assert bits(ra) == bits(rb) and bits(hs) == bits(np.zeros_like(hs))
        for k in hy.WRITES:
            assert bits(fa[k]) == bits(fb[k]), k
    # ... and in the mixed case the columns on no hillslope keep them too, the others do not
    m = G["down"] == -2
    on = wide[3]
    assert bits(on[1][1][:, m]) == bits(b[1][1][:, m]) and bits(on[1][0]["h2osoi_liq"][m]) == bits(b[1][0]["h2osoi_liq"][m])
    assert (on[1][1][hy.ZWT, ~m].view(np.uint64) != b[1][1][hy.ZWT, ~m].view(np.uint64)).sum() > 500


def test_a_flat_hillslope_moves_nothing():
    G = hc.slope5(flat=True)
    f, rows = hc.loam_fields(5, rain=1.0e-4)
    res = hy.step(f, rows, DT, lat=hc.lat_of(G))
    hs = res[2]
    assert bits(hs[hy.HS_HEAD]) == bits(np.zeros(5)) and (hs[hy.HS_TRANS] > 0.0).all()
    assert (hs[hy.HS_QLAT_OUT:] == 0.0).all()
    assert (res[1][hy.QFLX_DRAIN] == 0.0).all()  # L3 is wired to QLAT_NET: F.1's baseflow (rsub_top_max > 0) is gone
    plain = hy.step(f, rows, DT)
    assert (plain[1][hy.QFLX_DRAIN] > 0.0).all()
    # the stream column's head below zero: still nothing
    G["elev"] = G["elev"] - 1.0
    hs = hy.step(f, rows, DT, lat=hc.lat_of(G))[2]
    assert (hs[hy.HS_HEAD] == -1.0).all() and (hs[hy.HS_QLAT_OUT:] == 0.0).all()


def test_net_fluxes_sum_to_the_stream_discharge(wide):
    G, _, _, chain = wide
    for name in ("chain5", "star8"):
        g = hc.shape(name)
        cols, _, _, rows = hc.columns(g, 5)
        hs = hc.host_chain(g, cols, rows, 1)[0][2]
        res = abs(_fsum(g["area"] * 1.0e-3 * hs[hy.HS_QLAT_NET]) - _fsum(hs[hy.HS_QSTREAM]))
        # (area * 1e-3 * NET rounds twice more per column)
        bound = hc.l2_bound(g, hs) + 2.0 * U * float(np.abs(g["area"] * 1.0e-3 * hs[hy.HS_QLAT_NET]).sum())
        print(f"{name}: residual {float(res):.3e} m3/s, bound {bound:.3e}, sum QSTREAM {float(_fsum(hs[hy.HS_QSTREAM])):.3e}")
        assert res <= bound and float(_fsum(hs[hy.HS_QSTREAM])) > 1.0e6 * bound
    hs = chain[0][2]
    ok = np.isfinite(hs).all(axis=0)
    for c in np.nonzero(~ok)[0]:  # (a hillslope with a NaN in it is left out whole)
        j = int(c)
        while G["down"][j] >= 0:
            j = int(G["down"][j])
            ok[j] = False
    # every column of a left-out hillslope drains into a left-out column or is one
    for _ in range(12):
        ok[(G["down"] >= 0) & ~ok[np.maximum(G["down"], 0)]] = False
    net = np.where(ok, hs[hy.HS_QLAT_NET], 0.0)
    qs = np.where(ok, hs[hy.HS_QSTREAM], 0.0)
    res = abs(_fsum(G["area"] * 1.0e-3 * net) - _fsum(qs))
    bound = hc.l2_bound(G, np.where(ok, hs, 0.0)) + 2.0 * U * float(np.abs(G["area"] * 1.0e-3 * net).sum())
    print(f"wide: residual {float(res):.3e} m3/s, bound {bound:.3e}, sum QSTREAM {float(_fsum(qs)):.3e}, {int((~ok).sum())} columns left out")
    assert res <= bound and (~ok).sum() < 20
    assert bits(hy.hillslope_budget(qs)) == bits(np.array([diagnostics.reduce_min_max_sum(qs)[2]]))


# ---- the census ------------------------------------------------------------------------------------------------------------------------
def test_every_branch_is_taken_in_every_step_of_the_wide_case(wide):
    G, _, _, chain = wide
    for s, (_, rows, hs, hit) in enumerate(chain):
        assert set(hc.BRANCHES) <= hit, (s, set(hc.BRANCHES) - hit)
        assert {"drain_aquifer", "drain_soil"} <= hit
    # the edge values do what the statement says literally
    hs = chain[0][2]
    assert np.isnan(hs[hy.HS_HEAD, 80]) and hs[hy.HS_TRANS, 80] == 0.0 and np.isnan(hs[hy.HS_QLAT_IN, 81])  # NaN ZWT: jwt == N
    assert hs[hy.HS_HEAD, 82] == -INF and hs[hy.HS_TRANS, 82] == 0.0 and hs[hy.HS_HEAD, 84] == INF and hs[hy.HS_TRANS, 84] > 0.0
    assert hs[hy.HS_TRANS, 88] == 0.0 and hs[hy.HS_TRANS, 86] > hs[hy.HS_TRANS, 255] * 0.0
    assert 0.0 < hs[hy.HS_TRANS, 90] < 1.0e-5 * hs[hy.HS_TRANS, 91]  # the frozen column: impeded by 1e-6
    assert hs[hy.HS_QLAT_OUT, 255] > 0.0 and hs[hy.HS_QLAT_IN, 256] > 0.0


# ---- the budgets -----------------------------------------------------------------------------------------------------------------------
def _slope_chain(G, nsteps, on, rain=2.0e-4, evap=1.0e-5):
    f, rows = hc.loam_fields(G["ncols"], rain=rain, evap=evap)
    out = []
    for _ in range(nsteps):
        f = dict(f)
        f["dtbegin_column_h2o"] = water_mass(f)
        wb = hy.water_balance_begin(f, rows)
        res = hy.step(f, rows, DT, lat=hc.lat_of(G) if on else None)
        f.update(res[0])
        rows = res[1]
        wb = hy.water_balance_end(f, rows, wb, DT)
        out.append((f, rows, res[2] if on else None, wb))
    return out


def test_the_column_budget_keeps_its_error():
    """ERRH2O of every column of the loam slope over six chained steps, extension on: inside the counted bound of hillslope_cases.py; the
    lateral flux is far above it (the budget closes because QFLX_DRAIN carries the flux, not because the flux is small)."""
    G = hc.slope5()
    worst = 0.0
    for s, (f, rows, hs, wb) in enumerate(_slope_chain(G, 6, True)):
        e = float(np.abs(wb[hy.WB_ERRH2O]).max())
        worst = max(worst, e)
        print(f"step {s}: largest |ERRH2O| {e:.3e} mm, bound {hc.ERRH2O_BOUND:.3e}; largest |QLAT_NET| dt {float(np.abs(hs[hy.HS_QLAT_NET]).max()) * DT:.3e} mm")
        assert e <= hc.ERRH2O_BOUND
        assert float(np.abs(hs[hy.HS_QLAT_NET]).max()) * DT > 1.0e6 * hc.ERRH2O_BOUND
        assert float(water_mass(f).max() + rows[hy.WA].max()) < hc.W_MAX
        assert bits(rows[hy.QFLX_DRAIN]) == bits(hs[hy.HS_QLAT_NET])  # (no F.7 remainder on these columns)
    print(f"largest |ERRH2O| of the chain {worst!r} mm")
    assert worst <= hc.ERRH2O_MEASURED * 4.0 and hc.ERRH2O_MEASURED <= hc.ERRH2O_BOUND  # (the recorded value is this chain's)
    off = max(float(np.abs(wb[hy.WB_ERRH2O]).max()) for _, _, _, wb in _slope_chain(G, 6, False))
    assert off <= hc.ERRH2O_BOUND


def test_the_hillslope_budget_closes_with_the_stream_discharge():
    """Per step, in exact arithmetic: the hillslope's storage change, as volume, equals dt times (rain less evaporation less the surface
    runoff over the columns, less the stream discharge), up to the columns' own ERRH2O bound and consequence 3's roundings.  Without
    sum QSTREAM the identity misses the bound by orders of magnitude."""
    G = hc.slope5()
    vol = lambda x: sum((F(p) * F(q) / 1000 for p, q in zip(np.asarray(x).tolist(), G["area"].tolist())), F(0))  # noqa: E731
    worst = 0.0
    for s, (f, rows, hs, wb) in enumerate(_slope_chain(G, 6, True)):
        storage = vol(wb[hy.WB_ENDWB]) - vol(wb[hy.WB_BEGWB])
        external = F(DT) * (vol(f["forc_rain"]) - vol(f["qflx_evap_tot"]) - vol(rows[hy.QFLX_SURF]) - vol(rows[hy.QFLX_H2OSFC_SURF]))
        stream = F(DT) * _fsum(hs[hy.HS_QSTREAM])
        res = abs(storage - external + stream)
        bound = hc.hillslope_budget_bound(G, hs)
        worst = max(worst, float(res))
        print(f"step {s}: residual {float(res):.3e} m3, bound {bound:.3e} m3, sum QSTREAM dt {float(stream):.3e} m3")
        assert res <= bound, (s, float(res), bound)
        assert float(stream) > 1.0e6 * bound and abs(storage - external) > 1.0e6 * bound
        assert 0.99 * hc.HILLSLOPE_BUDGET_BOUND <= bound <= 1.01 * hc.HILLSLOPE_BUDGET_BOUND  # (the recorded bound is this chain's)
    print(f"largest residual of the chain {worst:.3e} m3")
    assert worst <= 4.0 * hc.HILLSLOPE_BUDGET_MEASURED and hc.HILLSLOPE_BUDGET_MEASURED <= hc.HILLSLOPE_BUDGET_BOUND


# ---- the physical check ----------------------------------------------------------------------------------------------------------------
def test_a_slope_from_equal_water_tables_ends_wet_at_the_toe():
    G = hc.slope5()
    on = _slope_chain(G, 96, True, rain=1.0e-4, evap=0.0)
    off = _slope_chain(G, 96, False, rain=1.0e-4, evap=0.0)
    zwt = on[-1][1][hy.ZWT]
    print("ZWT toe to ridge:", zwt.tolist(), "without:", off[-1][1][hy.ZWT].tolist())
    assert (np.diff(zwt) > 0.0).all()  # increasing from toe to ridge
    assert len(set(off[-1][1][hy.ZWT].tolist())) == 1  # equal without it
    assert on[-1][2][hy.HS_QSTREAM, 0] > 0.0 and (on[-1][2][hy.HS_QSTREAM, 1:] == 0.0).all()


def test_the_cost_tool_imports_without_device_or_library(tmp_path):
    """tests/tools/cost_hillslope.py imports without a device and without the built library, as tests/test_cost_tools_host.py asks of
    the *_cost.py tools, takes its protocol from costlib, and its geometries pass the checks with the map widths it names."""
    import sys

    tools = os.path.join(ROOT, "tests", "tools")
    src = open(os.path.join(tools, "cost_hillslope.py")).read()
    assert "import costlib as CL" in src and "perf_counter" not in src and "profiles/r28_hillslope_cost.jsonl" in src
    code = ("import sys, importlib\nsys.path.insert(0, sys.argv[1])\nm = importlib.import_module('cost_hillslope')\n"
            "from elmkernels_amd import hydrology as hy\n"
            "for s in m.SHAPES:\n"
            "    g = m.geometry(1003, s)\n"
            "    assert hy.hillslope_check(g[0], *(float(v) if isinstance(v, float) else v for v in g[1:5]), g[5])[0] is None, s\n"
            "    assert hy.hillslope_map(g[0]).shape[0] == m.MAP_WIDTH[s], s\n"
            "print('imported', m.CALLS == m.HC.CALLS, m.SHAPES, m.added_bytes('chain5')['head'])\n")
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, tools], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "imported True ('off', 'chain5', 'star8') 444", r.stderr[-2000:]


# ---- the header and the bindings ---------------------------------------------------------------------------------------------------------
ENTRY_POINTS = ("enable", "read", "budget", "clear")


def test_header_constants_and_bindings():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert h.index("int elmk_soil_hydrology_frost_clear(") < h.index("/* ---- hillslope lateral flow ----") < h.index("/* ---- water balance ----")
    assert ("enum { ELMK_HS_HEAD = 0, ELMK_HS_TRANS = 1, ELMK_HS_QLAT_OUT = 2, ELMK_HS_QLAT_IN = 3, ELMK_HS_QLAT_NET = 4, ELMK_HS_QSTREAM = 5, "
            "ELMK_HS_NROWS = 6 };") in h
    assert "enum { ELMK_ROWS_HILLSLOPE = 8 };" in h and st.ROWS_HILLSLOPE == 8 and st.ROW_FAMILIES["hillslope"] == 8
    names = (hy.HS_HEAD, hy.HS_TRANS, hy.HS_QLAT_OUT, hy.HS_QLAT_IN, hy.HS_QLAT_NET, hy.HS_QSTREAM)
    assert names == (st.HS_HEAD, st.HS_TRANS, st.HS_QLAT_OUT, st.HS_QLAT_IN, st.HS_QLAT_NET, st.HS_QSTREAM) == tuple(range(6))
    assert hy.HS_NROWS == st.HS_NROWS == 6
    for name in ENTRY_POINTS:
        assert re.search(rf"^int elmk_hillslope_{name}\(", h, re.M) and f"elmk_hillslope_{name}" in L.SIGNATURES, name
        assert hasattr(st.ELMState, "hillslope_" + name)
    assert hasattr(st.ELMState, "hillslope_rows")
    for k in (1, 2, 3):
        assert f" L{k} " in h
    hpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    for name in ENTRY_POINTS:
        assert f"elmk_hillslope_{name}(" in hpp, name
    # the kernels: a unit of its own without atomics and LDS; the hydrology kernel's LAT form beside the four forms it had
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_hillslope.hip")).read()
    assert "__global__ __launch_bounds__(256) void k_hillslope_head(" in k and "template <int NPAD>\n__global__ __launch_bounds__(256) void k_hillslope_flow(" in k
    assert "atomic" not in k.replace("no atomics", "") and "__shared__" not in k
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_soil_hydrology.hip")).read()
    first = k.index("template __global__ void k_soil_hydrology<false, false>(")
    assert first < k.index("template __global__ void k_soil_hydrology<true, true>(") < k.index("template __global__ void k_soil_hydrology_lat<LatRows>(")
    mk = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "Makefile")).read()
    assert "k_hillslope.hip" in mk and "api_hillslope.cpp" in mk
    # the texts of the checks are the same on both sides
    maps = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    for text in set(v.rsplit(" @", 1)[0] for v in REFUSALS.values()):
        assert f'"{text}"' in maps, text
