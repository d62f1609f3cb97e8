"""Stream temperature on the host (include/elmk.h "stream temperature"; elmkernels_amd/routing.py): H8 on the water rows; H7's closure
over ten chained calls against a bound counted from the statement's roundings; passive cells (no exchange through the surface): no
settle heat, no surface heat, and a confluence that mixes by flow; a still pool under constant forcing; the settle rule; the input
check in Python and through a stand-alone program, plain and under the address and undefined-behaviour sanitizers; the header's
constants and the bindings."""
import os
import re
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import heat_cases as hc
from tests.support import ROOT, bits

U = 2.0 ** -53
N = 211


def _forest(n=N, seed=5):
    """A forest of n cells with finite water (the edge values taken out), its map, columns and temperatures."""
    ddist, area, p, volr, wh, wt = hc.cell_values(n, 40 + n)
    fin = lambda x: np.where(np.isfinite(x) & (np.abs(x) < 1e200) & (x >= 0.0), x, 7.0)  # noqa: E731
    volr, wh, wt = (fin(x) for x in (volr, wh, wt))
    area = np.where(area > 0.0, area, 1.0e8)
    down = hc.networks(n, 52 + n)["forest"]
    shade, tt, tr = hc.heat_values(n, seed)
    tt, tr = (np.where((x > 200.0) & (x < 400.0), x, 280.0) for x in (tt, tr))
    return down, rt.upstream_map(down), area, p, (wh, wt, volr), shade, tt, tr


def test_the_water_rows_keep_their_bits():
    """H8: kinematic_call with and without heat= on the device test's forest, every branch of the heat in the call."""
    down, up, area, p, (wh, wt, volr), shade, tt, tr = _forest()
    ptr, col, w = hc.heat_map(N, 3)
    tab = rt.heat_tables(p, hc.SUBLEV, shade)
    qin, qsur = hc.aggregates(N, 9, 0)
    census = {}
    heat = {"tab": tab, "prep": rt.heat_prep(ptr, col, w, hc.columns(hc.NCOLS, 77), tab), "tt": tt, "tr": tr, "census": census}
    plain = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, 1800.0, 3)
    hot = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, 1800.0, 3, heat=heat)
    assert len(hot) == len(plain) + 7
    for a, b in zip(plain, hot):
        assert bits(a) == bits(b)
    assert not hc.missing_branches(census), hc.missing_branches(census)
    with pytest.raises(ValueError, match="heat with flood, dam or in_place"):
        rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, 1800.0, 3, heat=heat, dam={})
    with pytest.raises(ValueError, match="heat with flood, dam or in_place"):
        rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, 1800.0, 3, heat=heat, flood=({}, volr))


def test_the_budget_closes_over_ten_chained_calls():
    """H7 over ten chained calls of three sub-steps on a random forest under new forcing each call: per call
    sum HEAT_end - sum HEAT_start = sums[1] + sums[2] + sums[3] - sums[4], all six sums through heat_budget's reduction.

    The bound, counted in roundings (u = 2^-53).  In exact arithmetic on the doubles the call held the identity holds cell by cell and
    sub-step by sub-step: the tributaries' et * TT is the same double where it leaves (H3) and where it arrives (H4), and hr[c] is the
    same double in the cell's own ho and in its downstream cell's fh, so transport cancels and only the outlets' ho remains.  What is
    left are the roundings.  Per cell and sub-step the statement rounds at most: H3's h 9 times (TT * WT, eh * TSUR, gb, hi, et * TT,
    the three additions inside the bracket counted as 2, * dts, the outer +), H4's h 14 times (TR * VOLR, up to 8 additions of fh,
    fh - ho, + et * TT, + sx, * dts, the outer +; et * TT itself is counted above), the two settles 2 each (t * wn and - h where the
    rule acts; where it does not, t * wn differs from h by the division's rounding, 1 each), H6 9 times (hi * dts and its +=;
    sx_T + sx_R, * dts, +=; adj_T + adj_R, +=; ho * dts, +=), and HEAT's product pair and sum 3 times at a call's end: 40 in all.
    Every one of these rounds a partial result whose magnitude is at most A, the sum of the magnitudes of every term the cell's heat
    handles in the sub-step and of the four running diagnostics (kinematic_call's heat["mag"]), so the cells contribute at most
    40 u sum A.  Each of the six reductions over n cells adds n - 1 roundings of at most u sum |x| each; combining the four sums on
    the right takes 3 roundings of at most u (|s1| + |s2| + |s3| + |s4|) and the difference on the left one of u (|H1| + |H0|).
    Times 1.01 for the higher orders."""
    down, up, area, p, (wh, wt, volr), shade, tt, tr = _forest()
    ptr, col, w = hc.heat_map(N, 3)
    tab = rt.heat_tables(p, hc.SUBLEV, shade)
    nsub, dt = 3, 1800.0
    with np.errstate(all="ignore"):
        heat0 = tt * wt + tr * volr
    worst = 0.0
    for c in range(10):
        qin, qsur = hc.aggregates(N, 9, c)
        mag = []
        heat = {"tab": tab, "prep": rt.heat_prep(ptr, col, w, hc.columns(hc.NCOLS, 77, c, edges=False), tab), "tt": tt, "tr": tr, "mag": mag}
        out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, heat=heat)
        wh, wt, volr = out[:3]
        tt, tr, heat1, hin, hsrf, hadj, hout = out[4:]
        assert len(mag) == nsub and all(np.isfinite(x).all() for x in (heat1, hin, hsrf, hadj, hout))
        s = rt.heat_budget(heat1, hin, hsrf, hadj, hout, down)
        s0 = rt.heat_budget(heat0, hin, hsrf, hadj, hout, down)[0]
        lhs, rhs = s[0] - s0, s[1] + s[2] + s[3] - s[4]
        outlet = np.where(down < 0, hout, 0.0)
        reductions = (N - 1) * sum(np.abs(x).sum() for x in (heat1, heat0, hin, hsrf, hadj, outlet))
        bound = 1.01 * U * (40.0 * sum(m.sum() for m in mag) + reductions + 3.0 * np.abs(s[1:]).sum() + (abs(s[0]) + abs(s0)))
        assert bound < 1.0e-9 * abs(s[0])  # (the bound is about roundings: parts in 1e9 of the heat content would be no test)
        assert abs(lhs - rhs) <= bound, (c, lhs - rhs, bound)
        worst = max(worst, abs(lhs - rhs) / bound)
        assert abs(s[1]) > 1.0e3 and abs(s[2]) > 1.0e3 and abs(s[4]) > 1.0e3  # every path carries heat
        heat0 = heat1
    assert worst > 0.0  # (an identity that held exactly would compare nothing)


def _passive_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, tt, tr, tsur, tsub):
    n = volr.size
    heat = {"tab": rt.heat_tables(p), "prep": hc.passive_prep(n, tsur, tsub), "tt": tt, "tr": tr}
    return rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, heat=heat)


def test_passive_deep_water_has_no_settle_and_no_surface_heat():
    """RAD = KE = EMS = 0 (cells without terms) and water deep enough that the settle rule never acts: HADJ == 0 and HSRF == 0
    exactly, over five chained calls on the forest."""
    down, up, area, p, (wh, wt, volr), _, tt, tr = _forest()
    wt, volr = wt + 1.0e5, volr + 1.0e5  # every store far above WMINT / WMINR (at most 4e3 m3 here)
    tt, tr = np.clip(tt, 274.0, 300.0), np.clip(tr, 274.0, 300.0)
    rng = np.random.default_rng(2)
    tsur, tsub = rng.uniform(274.0, 300.0, N), rng.uniform(274.0, 300.0, N)
    for c in range(5):
        qin = np.random.default_rng(30 + c).uniform(0.5, 8.0, N)
        out = _passive_call(wh, wt, volr, qin, 0.4 * qin, area, p, up, 1800.0, 3, tt, tr, tsur, tsub)
        wh, wt, volr = out[:3]
        tt, tr, heat, hin, hsrf, hadj, hout = out[4:]
        tab = rt.heat_tables(p)
        assert (wt > tab["WMINT"]).all() and (volr > tab["WMINR"]).all()
        assert bits(hadj) == bits(np.zeros(N)) and bits(hsrf) == bits(np.zeros(N))
        assert (hin > 0.0).all() and (tt >= 274.0).all() and (tt <= 300.0).all() and (tr >= 274.0).all() and (tr <= 300.0).all()


def test_a_confluence_tends_to_the_flow_weighted_mean():
    """Two headwater cells of different runoff and runoff temperature into a third with no runoff of its own, passive cells, a steady
    inflow: the third cell's TR tends to (er_0 TR_0 + er_1 TR_1) / (er_0 + er_1).  Once the water is steady, a sub-step maps the
    distance to that mean by the factor 1 - er dts / VOLR of the slowest store on the way (explicit mixing of a store with its
    inflow), so after k sub-steps it is at most the first distance times rho^k, plus what the stores still upstream of it lag."""
    n = 3
    down = np.array([2, 2, -1], np.int32)
    up = rt.upstream_map(down)
    p, area = hc.uniform_params(n), np.full(n, 1.0e8)
    p[rt.RLEN] = 2.0e3  # (short reaches: the water of a reach is renewed in a few hours)
    qin = np.array([2.0, 6.0, 0.0])
    tsub = np.array([278.0, 296.0, 285.0])
    dt, nsub = 1800.0, 3
    ct, cr = rt.kinematic_params(p)[1:]

    def steady(q, length, width, c):  # the storage that releases q, by bisection on K4
        lo, hi = np.zeros(n), np.full(n, 1.0e9)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            below = rt.channel_flow(mid, length, width, c, dt / nsub) < q
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return hi

    wh, wt, volr = np.zeros(n), steady(qin, p[rt.TLEN], p[rt.TWIDTH], ct), steady(np.array([2.0, 6.0, 8.0]), p[rt.RLEN], p[rt.RWIDTH], cr)
    tt, tr = np.full(n, 285.0), np.full(n, 285.0)
    for _ in range(20):  # the water settles on its steady state
        wh, wt, volr, qout, tt, tr = _passive_call(wh, wt, volr, qin, np.zeros(n), area, p, up, dt, nsub, tt, tr, tsub, tsub)[:6]
    assert np.allclose(qout, [2.0, 6.0, 8.0], rtol=1e-9)
    mean = (2.0 * 278.0 + 6.0 * 296.0) / 8.0
    dist = []
    tt, tr = np.array([278.0, 296.0, 285.0]), np.array([278.0, 296.0, 280.0])  # the headwaters at their inflow's temperature
    rho = 1.0 - (8.0 * (dt / nsub)) / volr[2]
    assert 0.0 < rho < 1.0
    for k in range(120):
        wh, wt, volr, qout, tt, tr = _passive_call(wh, wt, volr, qin, np.zeros(n), area, p, up, dt, nsub, tt, tr, tsub, tsub)[:6]
        dist.append(abs(tr[2] - mean))
        assert dist[-1] <= abs(280.0 - mean) * rho ** (nsub * (k + 1)) + 1.0e-9
    assert dist[-1] < 1.0e-6 and abs(tr[0] - 278.0) < 1e-9 and abs(tr[1] - 296.0) < 1e-9


def _pool_prep(n=1):
    """One cell under a constant summer forcing, as heat_prep leaves it."""
    cols = {"forc_tbot": np.full(1, 293.0), "forc_pbot": np.full(1, 1.0e5), "forc_qbot": np.full(1, 8.0e-3), "forc_lwrad": np.full(1, 350.0),
            "forc_u": np.full(1, 3.0), "forc_v": np.full(1, 0.0), "forc_solad": np.full((1, 2), 120.0), "forc_solai": np.full((1, 2), 40.0),
            "t_grnd": np.full(1, 290.0), "t_soisno": np.full((1, 20), 288.0)}
    return cols


@pytest.mark.parametrize("start", [276.0, 310.0], ids=["from below", "from above"])
def test_a_still_pool_approaches_the_temperature_where_phi_vanishes(start):
    """One cell whose main channel hardly moves (a slope of 1e-300) holds a pool 0.2 m deep, no runoff: TR approaches the root of phi
    from the side it started on, monotonically, and ends within a thousandth of the first distance."""
    p = hc.uniform_params(1)
    p[rt.RSLP] = 1.0e-300
    tab = rt.heat_tables(p)
    x = rt.heat_prep(np.array([0, 1]), np.array([0], np.int32), np.array([1.0]), _pool_prep(), tab)
    lo, hi = 274.0, 312.0
    assert rt.heat_phi(np.array([lo]), x)[0] > 0.0 > rt.heat_phi(np.array([hi]), x)[0]
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if rt.heat_phi(np.array([mid]), x)[0] > 0.0 else (lo, mid)
    root = 0.5 * (lo + hi)
    volr = 0.2 * tab["ACHN"]
    up = rt.upstream_map(np.array([-1], np.int32))
    z = np.zeros(1)
    wh, wt, tt, tr = z, z, np.full(1, rt.TFRZ), np.full(1, start)
    d0 = prev = abs(start - root)
    for _ in range(150):
        out = rt.kinematic_call(wh, wt, volr, z, z, np.full(1, 1.0e8), p, up, 1800.0, 2, heat={"tab": tab, "prep": x, "tt": tt, "tr": tr})
        wh, wt, volr = out[:3]
        tt, tr = out[4:6]
        d = abs(tr[0] - root)
        assert (tr[0] - root) * (start - root) > 0.0 or d < 1.0e-9  # it stays on its side
        assert d < prev or d < 1.0e-9
        prev = d
        assert out[9][0] == 0.0  # HADJ: the settle rule never acts
    assert prev < 1.0e-3 * d0 and abs(volr[0] - 0.2 * tab["ACHN"][0]) < 1.0e-6 * volr[0]


def test_the_settle_rule():
    """A film below DMIN takes TEQ; a store driven below TFRZ or above TMAX is held there and adj carries the difference; a store that
    stays inside adds nothing."""
    wmin = np.full(5, 1.0e3)
    wn = np.array([999.0, 5.0e5, 5.0e5, 5.0e5, np.nan])
    h = np.array([999.0 * 290.0, 5.0e5 * 250.0, 5.0e5 * 330.0, 5.0e5 * 288.0, 1.0e8])
    teq = np.array([281.0, 281.0, 281.0, 281.0, 277.0])
    census = {}
    t, adj = rt.heat_settle(h, wn, wmin, teq, census)
    assert bits(t[:4]) == bits(np.array([281.0, rt.TFRZ, rt.TMAX, h[3] / wn[3]])) and t[4] == 277.0
    assert adj[0] == 281.0 * 999.0 - h[0] and adj[1] == rt.TFRZ * 5.0e5 - h[1] > 0.0 and adj[2] == rt.TMAX * 5.0e5 - h[2] < 0.0
    assert adj[3] == 0.0 and np.isnan(adj[4])
    assert [bool(census[k][i]) for k, i in (("settle TEQ", 0), ("settle TFRZ", 1), ("settle TMAX", 2), ("settle inside", 3), ("settle TEQ", 4))] == [True] * 5
    # a NaN heat content comes back to TFRZ
    t, adj = rt.heat_settle(np.array([np.nan]), np.array([5.0e5]), wmin[:1], teq[:1])
    assert t[0] == rt.TFRZ and np.isnan(adj[0])
    # in a call: a film in the tributaries under a cell without terms takes TEQ = TFRZ
    p = hc.uniform_params(1)
    tab = rt.heat_tables(p)
    film = 0.5 * tab["WMINT"]
    out = _passive_call(np.zeros(1), film, 2.0 * tab["WMINR"] + 1.0e5, np.zeros(1), np.zeros(1), np.full(1, 1.0e8), p,
                        rt.upstream_map(np.array([-1], np.int32)), 60.0, 1, np.full(1, 290.0), np.full(1, 290.0), None, None)
    assert out[4][0] == rt.TFRZ and out[9][0] != 0.0


# ---- the input check -------------------------------------------------------------------------------------------------------------------
def test_check_heat_refuses_what_the_entry_point_refuses():
    rt.check_heat(0), rt.check_heat(14, np.array([0.0, 1.0, 0.5, -0.0]))
    for s in (-1, 15, 99):
        with pytest.raises(ValueError, match=re.escape(rt.E_SUBLEV)):
            rt.check_heat(s, np.array([np.nan]))  # (sublev before shade)
    for bad in (np.nan, np.inf, -np.inf, -1e-300, 1.0000000000000002):
        shade = np.array([0.0, 0.5, bad, 0.5, np.nan])
        with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_SHADE, 2))):
            rt.check_heat(0, shade)
    with pytest.raises(ValueError, match="shade must be"):
        rt.check_heat(0, np.zeros(3), ncells=4)
    tab = rt.heat_tables(hc.uniform_params(3), 2, np.array([0.0, 1.0, 0.25]))
    assert bits(tab["KSW"]) == bits(np.array([0.9, 0.0, (1.0 - 0.1) * 0.75])) and tab["EMS0"] == (0.97 * 5.67e-8) / 4188000.0
    assert bits(tab["WMINT"]) == bits((hc.uniform_params(3)[rt.TLEN] * hc.uniform_params(3)[rt.TWIDTH]) * 1e-3)


def _build_checks(tmp_path, flags, name):
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "c", "heat_checks.cc")
    inc = os.path.join(ROOT, "elmkernels_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("flags", [(), ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")],
                         ids=["plain", "asan-ubsan"])
def test_the_host_check_as_a_program(tmp_path, flags):
    """tests/c/heat_checks.cc drives elmk_maps.h: heat_check: every refusal with the text and the cell check_heat gives, KSW bit for
    bit heat_tables', padding cells zero."""
    exe = _build_checks(tmp_path, flags, "heat_checks")
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    lines = dict(s.split(": ", 1) for s in out)
    assert lines["ncells 0"] == rt.E_NCELLS
    for name in ("sublev -1", "sublev 15", "sublev before shade"):
        assert lines[name] == rt.E_SUBLEV
    nbad = 0
    for name, text in lines.items():
        m = re.fullmatch(r"bad SHADE (\d) (\d)", name)
        if m:
            nbad += 1
            assert text == rt.e_cell(rt.E_SHADE, int(m.group(2))), name
    assert nbad == 6
    shade = np.array([0.0, 1.0, 0.25, 5e-324, 0.9999999999999999])
    p = hc.uniform_params(5)
    for name, s in (("valid", shade), ("null shade", None), ("negative zero", np.where(np.arange(5) == 2, -0.0, shade))):
        vals = lines[name].split()
        assert vals[0] == "ok" and len(vals) == 6, name
        assert bits(np.array([float.fromhex(v) for v in vals[1:]])) == bits(rt.heat_tables(p, 0, s)["KSW"]), name
    assert lines["sublev 14"] == "ok" and lines["sixty-five cells"] == "ok" and lines["short ld"] == "ok 5"
    assert lines["no outputs"] == f"ok / {rt.E_SHADE}"


# ---- the header and the bindings -----------------------------------------------------------------------------------------------------------
def test_the_header_the_bindings_and_the_constants_agree():
    text = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert ("enum { ELMK_ROUTE_TT = 13, ELMK_ROUTE_TR = 14, ELMK_ROUTE_HEAT = 15, ELMK_ROUTE_HIN = 16,\n"
            "       ELMK_ROUTE_HSRF = 17, ELMK_ROUTE_HADJ = 18, ELMK_ROUTE_HOUT = 19 };") in text
    assert (rt.TT, rt.TR, rt.HEAT, rt.HIN, rt.HSRF, rt.HADJ, rt.HOUT) == tuple(range(13, 20))
    assert (st.ROUTE_TT, st.ROUTE_TR, st.ROUTE_HEAT, st.ROUTE_HIN, st.ROUTE_HSRF, st.ROUTE_HADJ, st.ROUTE_HOUT) == tuple(range(13, 20))
    for name in ("enable", "init", "budget", "clear"):
        assert f"int elmk_routing_heat_{name}(elmk_ctx *ctx" in text and f"elmk_routing_heat_{name}" in L.SIGNATURES
        assert hasattr(st.ELMState, f"routing_heat_{name}")
    for k in range(10):
        assert f" * H{k}. " in text
    lit = re.search(r"Literals: (.*?)\n \*\n", text, re.S).group(1)
    for name in ("TFRZ", "TMAX", "RHOCP", "EMIS", "SB", "ALBW", "CPAIR", "LV", "RAIR", "CEX", "DMIN"):
        assert float(re.search(rf"\b{name} = ([0-9.e+-]+?)[,.]?\s", lit).group(1)) == getattr(rt, name), name
    maps = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    for msg in (rt.E_SUBLEV, rt.E_SHADE):
        assert f'"{msg}"' in maps
    from elmkernels_amd import restart as R
    assert R.VERSION_HEAT == 8 and "enum { ELMK_RESTART_VERSION_HEAT = 8 };" in text
