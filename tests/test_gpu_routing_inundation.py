"""Floodplain inundation on the device (include/elmk.h "floodplain inundation"): k_kinematic_step's flood form against the host
restatement (routing.kinematic_call(flood=...), inundation_tables, inundation_exchange) bit for bit on all ten rows, in both builds,
over five chained calls on every network shape, size, nsub and dt, with every path of I1 - I4 in every call and the edge values in
cells of their own; the edge values by value against a scalar reading of I1 - I4; the stage inside elmk_run against the stepwise calls,
graph on and off, with the extension switched between runs; restarts; the clear; the interlocks; every refusal; the budget; the river
supply limit; the example."""
import ctypes as C
import functools

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc
from tests import river_cases as rv
from tests.hydrology_cases import _new, prepare
from tests.irrigation_cases import generated
from tests.river_cases import NCELL, NSTEPS, TOL, differing, finite, host_inputs, read_rows, river_snapshot, set_runoff
from tests.run_cases import DT, NREC, assert_same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR, rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC)
NAMES = ("VOLR", "QIN", "QOUT", "QOUT_SUM", "WH", "WT", "QSUR", "WF", "FLOOD_DEPTH", "FLOOD_FRAC")
NAN, INF = ic.NAN, ic.INF


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return rv.base()


def enable_all(D, down, ddist, area, p, rdepth, eprof, nsub):
    D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
    D.routing_kinematic_enable(p)
    D.routing_inundation_enable(rdepth, eprof)


_ctx = functools.partial(rv.context, cell_map=ic.cell_map)


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 257, 1001])
def test_five_chained_calls_equal_the_restatement(base, ncells, lib_path):
    """Per network shape and (nsub, dt): enable all three, init with the edge values, five calls with a new runoff row before each;
    after every call all ten rows against routing.kinematic_call(flood=...) on what the device held before it, bit for bit.

    The census, on the restatement (inundation_cases.call_census, sub-step by sub-step): from 257 cells on every call of every
    network and case holds an untouched cell, a cell that returns its water (I2), a cell in each of the ten segments and a cell above
    the profile among cells 192 .. 319, which are the last wave of the first workgroup and the first of the second (at 257 cells: cells
    192 .. 256, one wave and the cell across the boundary).  inundation_cases.flood_values says how the cells are made to hold their
    paths through five calls.  At 63, 64 and 65 cells the same thirteen paths are asserted over the calls of the test together, not in
    every call: 1e300 and +inf from the edge cells travel a cell per sub-step and cover a chain of 63 cells inside the fifteen to
    forty sub-steps of a case, and a cell that holds 1e300 is above the profile whatever its banks."""
    D = _ctx(base, lib_path, ncells)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    bytes0 = D.device_bytes
    qs = [set_runoff(D, ic.snwcp(c)) for c in range(3)]  # (three runoff rows serve the five calls in turn)
    hosts = [host_inputs(D, q, area) for q in qs]
    cld = (ncells + 63) // 64 * 64
    union, widths = np.zeros(len(ic.PATHS), bool), set()
    lo, hi = ic.WINDOW[0], min(ncells, ic.WINDOW[1])
    for name, down in ic.networks(ncells, 52 + ncells).items():
        up = rt.upstream_map(down)
        widths.add(rt.npad_of(up))  # the NPAD the launch picks its kernel by
        for nsub, dt in ic.CASES:
            rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(ncells, 60 + ncells, area, p0, volr0, wh0, wt0, nsub, dt, rbank=1.0e6)
            tab = rt.inundation_tables(area, p, rdepth, eprof)
            D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
            D.routing_kinematic_enable(p)
            bytes2 = D.device_bytes
            D.routing_inundation_enable(rdepth, eprof)
            assert D.device_bytes - bytes2 >= (3 + 25) * 8 * cld
            assert not any(r.any() for r in read_rows(D, ROWS))
            D.routing_init(volr)
            D.routing_kinematic_init(wh, wt)
            D.routing_inundation_init(wf)
            qsum = np.zeros(ncells)
            for c in range(ic.NCALLS):
                D.upload("qflx_snwcp_liq", ic.snwcp(c % 3))  # the row the call reads is the water balance's of this moment
                D.water_balance(DT)
                D.routing(dt)
                qin, qsur, _ = hosts[c % 3]
                seen = ic.call_census(wh, wt, volr, wf, qin, qsur, area, p, up, dt, nsub, tab)
                union |= seen.any(axis=0)
                if ncells >= 257:
                    held = seen[lo:hi].any(axis=0)
                    assert held.all(), (name, nsub, dt, c, [ic.PATHS[i] for i in np.nonzero(~held)[0]])
                wh, wt, volr, qout, wf, depth, frac = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, flood=(tab, wf))
                with np.errstate(all="ignore"):
                    qsum = rt._canon(qsum + qout)
                for g, want, what in zip(read_rows(D, ROWS), (volr, qin, qout, qsum, wh, wt, qsur, wf, depth, frac), NAMES):
                    assert bits(g) == bits(want), (name, nsub, dt, c, what, differing(g, want))
                assert D.routing_count() == c + 1
            if ncells > 1:
                part = D.routing_read(rt.WF, cell0=ncells // 2, n=ncells - ncells // 2)
                assert bits(part) == bits(wf[ncells // 2:])
            D.routing_clear()  # frees all three
            assert D.device_bytes == bytes0
    if ncells >= 63:
        assert union.all(), [ic.PATHS[i] for i in np.nonzero(~union)[0]]
        assert widths == {1, 2, 4, 8}, widths  # every instantiation with_npad can pick
    D.close()


# ---- 2. the edge values, by value ------------------------------------------------------------------------------------------------------
def exchange_scalar(v, wf, c, tab, area):
    """I1 - I4 read literally for one cell, in Python floats (IEEE doubles, no contraction).  Returns (VOLR, WF, FLOOD_DEPTH,
    FLOOD_FRAC)."""
    vc, achn, af = float(tab["VC"][c]), float(tab["ACHN"][c]), float(tab["AF"][c])
    e, vb = [float(x) for x in tab["E"][:, c]], [float(x) for x in tab["VB"][:, c]]
    if not (wf > 0.0 or v > vc):
        return v, wf, 0.0, 0.0
    w = v + wf
    if not (w > vc):
        return w, 0.0, 0.0, 0.0
    x = w - vc
    if x >= vb[10]:
        s10 = achn + af * (10.0 / 10.0)
        d = x - vb[10]
        h, f = (e[10] + d / s10) if d == d else NAN, 1.0
    else:
        k = max(j for j in range(10) if x >= vb[j])
        fk = float(k) / 10.0
        sk, de = achn + af * fk, e[k + 1] - e[k]
        mk = (af * 0.1) / de
        r = x - vb[k]
        d = (2.0 * r) / (sk + float(np.sqrt(sk * sk + (2.0 * mk) * r)))
        if d > de:
            d = de
        h, f = e[k] + d, fk + (0.1 * d) / de
    vc2 = vc + achn * h
    if vc2 > w:
        vc2 = w
    with np.errstate(all="ignore"):
        rest = float(np.float64(w) - np.float64(vc2))
    return vc2, rest, h, ((af * f) / area if area > 0.0 else 0.0)


def test_the_edge_values_do_what_the_statement_says(base):
    """One call of one sub-step on cells without upstream, so that K6's VOLR is known: every edge value in VOLR (cells 1, 3 .. 15, dry
    floodplains) and in WF (cells 2, 4 .. 16), a NaN floodplain over a river above its banks, a NaN river under a wet floodplain, a
    negative floodplain that pulls a river above its banks back under them, a cell of no area and a 40 m channel: by kind, as I8 lists
    them, and by value against exchange_scalar."""
    n, dt = 257, 1800.0
    D = _ctx(base, None, n)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(n, 40 + n)
    rdepth, eprof, p, volr0, wh0, wt0, wf0 = ic.flood_values(n, 60 + n, area, p0, volr0, wh0, wt0, 1, dt)
    rdepth[:24] = 5.0
    p[rt.NR, [56, 57, 58]] = 400.0  # (these three release next to nothing, so K6 leaves them where they are put)
    tab = rt.inundation_tables(area, p, rdepth, eprof)
    vc = tab["VC"]
    for c, (v, w) in {56: (2.0 * vc[56], NAN), 57: (NAN, 5.0), 58: (vc[58] + 1.0e4, -3.5e4), 18: (3.0 * vc[18], 0.0), 19: (2.0 * vc[19], 4.0e6)}.items():
        volr0[c], wf0[c] = v, w
    wt0[[56, 57, 58]] = 0.0
    down = ic.networks(n, 1)["outlets"]
    enable_all(D, down, ddist, area, p, rdepth, eprof, 1)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_inundation_init(wf0)
    set_runoff(D, ic.snwcp(0))
    D.routing(dt)
    v, _, qout, _, _, _, _, wf, depth, frac = read_rows(D, ROWS)
    ch, ct, cr = rt.kinematic_params(p)
    et0 = rt.channel_flow(wt0, p[rt.TLEN], p[rt.TWIDTH], ct, dt)
    er0 = rt.channel_flow(volr0, p[rt.RLEN], p[rt.RWIDTH], cr, dt)
    with np.errstate(all="ignore"):
        k6 = volr0 + ((0.0 - er0) + et0) * dt
    for c in list(range(1, 24)) + [56, 57, 58]:
        want = exchange_scalar(float(k6[c]), float(wf0[c]), c, tab, float(area[c]))
        got = (v[c], wf[c], depth[c], frac[c])
        assert bits(rt._canon(np.array(got))) == bits(rt._canon(np.array(want))), (c, got, want)
    zero = lambda c: wf[c] == 0.0 and not np.signbit(wf[c]) and depth[c] == 0.0 and frac[c] == 0.0  # noqa: E731
    # VOLR's edge values over a dry floodplain: zero, negative zero, negative, denormal, NaN and -inf are untouched (I1); +inf has released
    # +inf and left NaN before the exchange sees it; 1e300 stands above the profile
    for c in (1, 3, 5, 7, 11, 13, 15):
        assert zero(c) and bits(v[c:c + 1]) == bits(rt._canon(k6[c:c + 1])), c
    assert np.isnan(v[11]) and np.isnan(v[13]) and v[15] == -INF and qout[13] == INF
    assert k6[9] > 1e299 and v[9] > 1e296 and wf[9] > 0.9 * k6[9] and depth[9] > 1e290 and frac[9] == (tab["AF"][9] * 1.0) / area[9] and 0.97 < frac[9] < 1.0
    # WF's edge values under a river inside its banks: zero, negative zero, negative, NaN and -inf are untouched and keep their bits; the
    # denormal returns (I2) and leaves +0.0; 1e300 stands above the profile; +inf leaves inf - inf
    assert (k6[[2, 4, 6, 8, 12, 16]] <= vc[[2, 4, 6, 8, 12, 16]]).all()
    for c in (2, 4, 6, 12, 16):
        assert bits(wf[c:c + 1]) == bits(wf0[c:c + 1]) and v[c] == k6[c] and depth[c] == 0.0 and frac[c] == 0.0, c
    assert np.signbit(wf[4]) and wf[6] == -3.5e4 and np.isnan(wf[12]) and wf[16] == -INF
    assert zero(8) and v[8] == k6[8]
    assert v[10] > 1e297 and wf[10] > 0.9e300 and v[10] + wf[10] == 1e300
    assert v[14] == INF and np.isnan(wf[14]) and depth[14] == INF and frac[14] == tab["AF"][14] / area[14]
    # a NaN on either side of W takes I2; a negative floodplain is added like any other
    assert np.isnan(v[56]) and zero(56) and np.isnan(v[57]) and zero(57)
    assert k6[58] > vc[58] and v[58] == k6[58] + -3.5e4 and v[58] < vc[58] and zero(58)
    # no area: no floodplain, the water stands in the channel's prism and the fraction is 0; the 40 m channel spills like any other
    assert tab["AF"][18] == 0.0 and depth[18] > 0.0 and frac[18] == 0.0 and wf[18] <= 2.0 * np.spacing(v[18])
    assert depth[19] > 0.0 and wf[19] > 0.0 and 0.0 < frac[19] < 1.0
    D.close()


# ---- 3. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING


@pytest.fixture(scope="module")
def run_base():
    return rv.run_case(flood=True)


_run_context = functools.partial(rv.run_context, parts=("routing", "kinematic", "inundation"))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the flag and the extension on against the stepwise calls in every field and row, then a second run
    (on the captured step when the graph is on) against six more; the extension switched off between two runs, which drops the captured
    step and runs the plain form, and on again, which brings the flood form back; floodplains wet throughout."""
    steps = schedule(2 * NSTEPS)
    rdepth, eprof = run_base["rdepth"], run_base["eprof"]
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    a = river_snapshot(A, ROWS)
    assert_same(river_snapshot(B, ROWS), a)
    r = a["route"]
    assert (r[7] > 0.0).any() and (r[8] > 0.0).any() and (r[9] > 0.0).any() and (r[7] == 0.0).any() and B.routing_count() == NSTEPS
    stepwise(A, run_base["rec"], steps[NSTEPS:], FLAGS)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(river_snapshot(B, ROWS), river_snapshot(A, ROWS))
    wf = A.routing_read(rt.WF)
    for X in (A, B):
        X.routing_inundation_clear()
    stepwise(A, run_base["rec"], steps[:2], FLAGS)
    B.run(DT, steps[:2], FLAGS)
    assert_same(river_snapshot(B, ROWS[:7]), river_snapshot(A, ROWS[:7]))
    for X in (A, B):
        X.routing_inundation_enable(rdepth, eprof)
        X.routing_inundation_init(wf)
    stepwise(A, run_base["rec"], steps[2:4], FLAGS)
    B.run(DT, steps[2:4], FLAGS)
    a = river_snapshot(A, ROWS)
    assert_same(river_snapshot(B, ROWS), a)
    assert (a["route"][7] > 0.0).any() and B.routing_count() == 2 * NSTEPS + 4
    for X in (A, B):
        X.close()


# ---- 4. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it VOLR, QOUT_SUM, the count, WH, WT and WF; a fresh context, restart_load,
    routing_init, routing_kinematic_init, routing_inundation_init, three more steps: the bits of six steps in one context on all ten
    rows.  The image is the one a context without the extension saves."""
    steps = schedule(NSTEPS)
    A = _run_context(run_base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, ROWS)
    size_a = A.restart_size()
    A.close()
    B = _run_context(run_base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    img, count = B.restart_save(), B.routing_count()
    volr, qsum, wh, wt, wf = read_rows(B, (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF))
    assert count == 3 and B.restart_size() == size_a and (wf > 0.0).any()
    B.close()
    Cx = _run_context(run_base, True, lib_path, init=False)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.routing_kinematic_init(wh, wt)
    Cx.routing_inundation_init(wf)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, ROWS), want)
    # each init leaves the other entries' rows alone; inundation_init without a row zero-fills
    Cx.routing_init(volr, qsum, 2)
    Cx.routing_kinematic_init(wh, wt)
    assert bits(Cx.routing_read(rt.WF)) == bits(want["route"][7]) and bits(Cx.routing_read(rt.FLOOD_FRAC)) == bits(want["route"][9])
    Cx.routing_inundation_init()
    assert not any(Cx.routing_read(w).any() for w in (rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC))
    assert bits(Cx.routing_read(rt.VOLR)) == bits(volr) and bits(Cx.routing_read(rt.WH)) == bits(wh) and Cx.routing_count() == 2
    N = _run_context(run_base, True, lib_path, parts=("routing", "kinematic"))
    assert N.restart_size() == size_a
    N.close()
    Cx.close()


# ---- 5. the clear, the interlocks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_clear_returns_to_the_channel_without_banks(base, lib_path):
    """Three calls with the extension, inundation_clear, two calls without: on the seven kinematic rows the bits of a context that
    never had it, given the same VOLR, WH, WT, QOUT_SUM and count.  While it is on kinematic_clear is refused and changes nothing;
    routing_clear frees all three allocations."""
    n = 257
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(n, 40 + n)
    rdepth, eprof, p, volr0, wh0, wt0, wf0 = ic.flood_values(n, 60 + n, area, p0, volr0, wh0, wt0, 3, 1800.0)
    down = ic.networks(n, 52 + n)["forest"]
    A, B = _ctx(base, lib_path, n), _ctx(base, lib_path, n)
    bytes0 = A.device_bytes
    for D in (A, B):
        D.routing_enable(down, ddist, area, rt.EFFVEL, 3)
        D.routing_kinematic_enable(p)
        set_runoff(D, ic.snwcp(0))
    bytes_kw = A.device_bytes
    A.routing_inundation_enable(rdepth, eprof)
    bytes_fp = A.device_bytes
    assert bytes_fp - bytes_kw >= 28 * 8 * 320
    A.routing_init(volr0)
    A.routing_kinematic_init(wh0, wt0)
    A.routing_inundation_init(wf0)
    for _ in range(3):
        A.routing(1800.0)
    rows = read_rows(A, ROWS)
    assert (rows[7] > 0.0).any() and bits(rows[0]) != bits(volr0)
    with pytest.raises(L.ElmkError, match="elmk_routing_inundation_clear first"):
        A.routing_kinematic_clear()
    assert A.device_bytes == bytes_fp
    for g, h in zip(read_rows(A, ROWS), rows):
        assert bits(g) == bits(h)
    A.routing_inundation_clear()
    A.routing_inundation_clear()  # nothing to free: OK
    assert A.device_bytes == bytes_kw == B.device_bytes and A.routing_count() == 3
    for g, h in zip(read_rows(A, ROWS[:7]), rows):
        assert bits(g) == bits(h)
    with pytest.raises(L.ElmkError, match="unknown row"):
        A.routing_read(rt.WF)
    B.routing_init(rows[0], rows[3], 3)
    B.routing_kinematic_init(rows[4], rows[5])
    qin, qsur, _ = host_inputs(A, A.water_balance_read(hy.WB_QRUNOFF), area)
    wh, wt, v = rows[4], rows[5], rows[0]
    for _ in range(2):
        for D in (A, B):
            D.routing(1800.0)
        wh, wt, v, qout = rt.kinematic_call(wh, wt, v, qin, qsur, area, p, rt.upstream_map(down), 1800.0, 3)
    for g, h in zip(read_rows(A, ROWS[:7]), read_rows(B, ROWS[:7])):
        assert bits(g) == bits(h)
    assert bits(A.routing_read(rt.VOLR)) == bits(v) and bits(A.routing_read(rt.QOUT)) == bits(qout) and A.routing_count() == 5
    # ... and on again: the rows come back zero-filled, VOLR stays; kinematic_clear works once the extension is off
    A.routing_inundation_enable(rdepth, eprof)
    assert not any(A.routing_read(w).any() for w in ROWS[7:]) and bits(A.routing_read(rt.VOLR)) == bits(v)
    A.routing_clear()  # frees all three
    assert A.device_bytes == bytes0
    B.routing_kinematic_clear()
    B.routing_clear()
    assert B.device_bytes == bytes0
    A.close()
    B.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(run_base):
    """Every refusal of the four entries and of the interlock, with nothing changed by any; elmk_device_bytes and elmk_restart_size
    return to their figures after the clear."""
    b, rows, m, down, ddist, area, rdepth, eprof, p, volr, wh, wt, wf = (run_base[k] for k in ("b", "rows", "map", "down", "ddist", "area", "rdepth", "eprof", "p", "volr", "wh", "wt", "wf"))

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    D = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    D.set_graph(True)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    bytes0, size0 = D.device_bytes, D.restart_size()
    refused(lambda: D.routing_inundation_enable(rdepth, eprof), D.routing_inundation_init, D.routing_inundation_budget, match="not enabled")
    D.routing_inundation_clear()  # nothing to free: OK
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr)
    refused(lambda: D.routing_inundation_enable(rdepth, eprof), D.routing_inundation_init, D.routing_inundation_budget,
            match="the scheme is not on")
    assert D.device_bytes > bytes0
    D.routing_kinematic_enable(p)
    D.routing_kinematic_init(wh, wt)
    bytes1 = D.device_bytes
    state1 = river_snapshot(D, ROWS[:7])
    refused(D.routing_inundation_init, D.routing_inundation_budget, match="the extension is not on")
    refused(*(lambda w=w: D.routing_read(w) for w in ROWS[7:]), lambda: D.routing_read(10), match="unknown row")
    for v in (0.0, -0.0, -1.0, NAN, INF, -INF):
        r = rdepth.copy()
        r[11] = v
        refused(lambda r=r: D.routing_inundation_enable(r, eprof), match="elmk_routing_inundation_enable: RDEPTH not finite and > 0 at cell 11$")
    for k in range(rt.NPROF):
        for v in (NAN, INF, -INF):
            e = eprof.copy()
            e[k, 17] = v
            refused(lambda e=e: D.routing_inundation_enable(rdepth, e), match="elmk_routing_inundation_enable: EPROF not finite at cell 17$")
    e = eprof.copy()
    e[0, 5] = 1.0e-3
    refused(lambda: D.routing_inundation_enable(rdepth, e), match=r"elmk_routing_inundation_enable: EPROF\[0\] not 0 at cell 5$")
    for k in range(1, rt.NPROF):
        for step in (0.0, -0.5):
            e = eprof.copy()
            e[k, 17] = e[k - 1, 17] + step
            refused(lambda e=e: D.routing_inundation_enable(rdepth, e), match="elmk_routing_inundation_enable: EPROF not increasing at cell 17$")
    rc_, ec_ = np.ascontiguousarray(rdepth), np.ascontiguousarray(eprof)
    rp, ep = rc_.ctypes.data_as(C.c_void_p), ec_.ctypes.data_as(C.c_void_p)
    for args in ((None, ep), (rp, None)):
        assert D.lib.elmk_routing_inundation_enable(D.ctx, *args) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap:
        rc = D.lib.elmk_routing_inundation_enable(D.ctx, rp, ep)
        cap.end()
        assert rc == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    for call in (lambda: D.routing_inundation_enable(rdepth[:-1], eprof), lambda: D.routing_inundation_enable(rdepth, eprof[:, :-1]),
                 lambda: D.routing_inundation_enable(rdepth, eprof[:-1])):
        with pytest.raises(ValueError):
            call()
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS[:7]), state1)

    D.routing_inundation_enable(rdepth, eprof)
    bytes2 = D.device_bytes
    assert bytes2 > bytes1 and D.restart_size() == size0  # the image is what it was
    D.routing_inundation_init(wf)
    state2 = river_snapshot(D, ROWS)
    refused(lambda: D.routing_inundation_enable(rdepth, eprof), match="already on")
    refused(D.routing_kinematic_clear, match="elmk_routing_inundation_clear first")
    refused(lambda: D.routing_read(10), lambda: D.routing_read(-1), lambda: D.routing_read(rt.WF, cell0=NCELL, n=1))
    with pytest.raises(ValueError):
        D.routing_inundation_init(np.zeros(NCELL + 1))
    assert D.lib.elmk_routing_inundation_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap:
        rcs = (D.lib.elmk_routing_inundation_clear(D.ctx), D.lib.elmk_routing_inundation_init(D.ctx, None),
               D.lib.elmk_routing_inundation_budget(D.ctx, rp))
        cap.end()
        assert rcs == (-1, -1, -1) and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes2 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS), state2)
    # the following step is the step of a context that met no refusal
    W = _run_context(run_base, True, nsub=2)
    for X in (D, W):
        X.run(DT, schedule(1), FLAGS)
    assert_same(river_snapshot(D, ROWS), river_snapshot(W, ROWS))
    D.routing_inundation_clear()
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    D.routing_inundation_enable(rdepth, eprof)
    D.routing_clear()  # frees all three
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    refused(lambda: D.routing_inundation_enable(rdepth, eprof), match="not enabled")
    D.close()
    W.close()


# ---- 7. the budget -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [1, 65, 1001])
def test_budget_equals_the_restatement(base, ncells):
    D = _ctx(base, None, ncells)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    volr0, wh0, wt0 = (finite(x) for x in (volr0, wh0, wt0))
    rdepth, eprof, p, volr0, wh0, wt0, wf0 = ic.flood_values(ncells, 60 + ncells, area, p0, volr0, wh0, wt0, 2, 1800.0)
    wf0 = finite(wf0)
    if ncells == 1:
        volr0, wf0 = volr0 + 1.0e8, wf0 + 1.0e6
    down = ic.networks(ncells, 5)["forest" if ncells >= 3 else "outlets"]
    enable_all(D, down, ddist, area, p, rdepth, eprof, 2)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_inundation_init(wf0)
    q = ic.snwcp(1)
    q[9] = 2.0e-5
    set_runoff(D, q)
    for _ in range(2):
        D.routing(1800.0)
    rows = read_rows(D, ROWS)
    want, want_kw, want_fp = rt.budget(rows[0], rows[1], rows[2], down), rt.kinematic_budget(rows[4], rows[5]), rt.inundation_budget(rows[7])
    assert np.isfinite(want).all() and np.isfinite(want_kw).all() and np.isfinite(want_fp).all() and want_fp[0] > 0.0
    for _ in range(2):  # (in turn: the three share the reduction's scratch)
        assert bits(D.routing_inundation_budget()) == bits(want_fp)
        assert bits(D.routing_kinematic_budget()) == bits(want_kw)
        assert bits(D.routing_budget()) == bits(want)
    for g, h in zip(read_rows(D, ROWS), rows):
        assert bits(g) == bits(h)  # (the calls change no row)
    D.close()


# ---- 8. the river supply limit -------------------------------------------------------------------------------------------------------
def test_the_supply_limit_reads_the_channel_not_the_floodplain():
    """The irrigation's river supply limit reads the VOLR row, which after a call is the channel's share: a context whose rivers stand
    over their banks grants what a context without the extension grants from the same VOLR row, bit for bit on the limit's four rows and
    on RATE, and not what it would grant if the floodplain's water counted."""
    n, ncells = 600, 65
    cols, scal, soil, sched = generated(n, 900)
    rows = prepare(cols, 613)
    m = sc.cell_map(n, ncells, 51, empty=(0,), single=(5, 7))
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, 9)
    p = np.repeat(np.array(ic.BASE)[:, None], ncells, axis=1)
    rdepth, eprof = np.full(ncells, 0.5), np.repeat((0.3 * np.arange(11))[:, None], ncells, axis=1)
    down = np.full(ncells, -1, np.int32)
    vc = rt.inundation_tables(area, p, rdepth, eprof)["VC"]
    ctxs = []
    for k in range(3):
        D = _new(cols, scal, soil, rows, None)
        D.water_balance_enable(TOL)
        D.set_output_grid(*m, fill=NAN)
        D.irrigation_enable(sched)
        D.irrigation_init(np.where(sched >= 0, 3.0e-3, 0.0), np.where(np.arange(n) % 3 == 0, 4.0, 0.0))
        D.routing_enable(down, ddist, area, rt.EFFVEL, 1)
        D.routing_set_withdrawal(True)
        D.routing_kinematic_enable(p)
        D.irrigation_supply_enable(0.1)
        ctxs.append(D)
    A, B, W = ctxs
    A.routing_inundation_enable(rdepth, eprof)
    A.routing_init(1.02 * vc)
    A.routing_inundation_init(np.full(ncells, 3.0e5))
    for D in ctxs:
        st.kokkos_init_timestep(D)
        D.water_balance_begin()
        st.timestep7_fused(D, DT)
        D.soil_hydrology(DT)
        D.water_balance(DT)
    A.routing(DT)
    volr, wf = A.routing_read(rt.VOLR), A.routing_read(rt.WF)
    assert (wf > 0.0).sum() >= ncells - 1 and (volr > 0.0).all()  # (cell 18 has no area and so no floodplain)
    B.routing_init(volr)
    W.routing_init(volr + wf)
    for D in ctxs:
        D.irrigation(DT, 12 * 3600)
    sup = [np.stack([D.irrigation_supply_read(k) for k in (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)]) for D in ctxs]
    rate = [D.irrigation_rows()[ir.RATE] for D in ctxs]
    assert bits(sup[0]) == bits(sup[1]) and bits(rate[0]) == bits(rate[1])
    assert (sup[0][ir.RATIO] < 1.0).any() and bits(sup[0][ir.RATIO]) != bits(sup[2][ir.RATIO])
    assert bits(A.routing_read(rt.VOLR)) == bits(volr) and bits(A.routing_read(rt.WF)) == bits(wf)  # (the limit only reads)
    for D in ctxs:
        D.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_inundation_demo(tmp_path):
    """examples/inundation_demo.cc builds with g++ against the C ABI and runs: 48 steps with and without banks, both outlets
    discharge, the banks flood and hold the peak back."""
    out = run_demo(build_demo("inundation_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(48))
    plain, banks, frac = (np.array([float(s[k]) for s in steps]) for k in (2, 3, 4))
    assert plain.max() > 0.0 and banks.max() > 0.0 and (plain >= 0.0).all() and (banks >= 0.0).all()
    assert banks.max() <= plain.max() and (frac >= 0.0).all() and (frac < 1.0).all()
    assert sum(s.startswith("largest flooded fraction per cell:") for s in out) == 1
    most = np.array([float(x) for x in next(s for s in out if s.startswith("largest flooded fraction")).split(":")[1].split()])
    assert most.size == 8 and (most > 0.0).any() and not np.array_equal(plain, banks)
