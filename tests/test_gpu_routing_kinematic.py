"""Kinematic-wave routing on the device (include/elmk.h "kinematic-wave routing"): k_kinematic_prep and k_kinematic_step against the host
restatement (routing.kinematic_call, qin_from_rows, qsur_from_rows) bit for bit on all seven rows, in both builds, over five chained
calls on every network shape, size, nsub and dt with the edge values in cells of their own; the edge values by value; the stage inside
elmk_run against the stepwise calls, graph on and off; restarts through read / init / kinematic_init; switching back to the linear
scheme; the withdrawal on and off with the scheme on; both budgets; every refusal; a context that never turns the scheme on."""
import ctypes as C
import functools

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import river_cases as rv
from tests.hydrology_cases import _new, prepare
from tests.irrigation_cases import generated
from tests.routing_kinematic_cases import CASES, cell_map, cell_values, flow_census, networks, snwcp
from tests.river_cases import NCELL, NSTEPS, TOL, host_inputs, read_rows, river_snapshot, set_runoff
from tests.run_cases import DT, assert_same, schedule, stepwise
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR)
NAMES = ("VOLR", "QIN", "QOUT", "QOUT_SUM", "WH", "WT", "QSUR")
NAN, INF = float("nan"), float("inf")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return rv.base()


_ctx = rv.context


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 257, 1001])
def test_five_chained_calls_equal_the_restatement(base, ncells, lib_path):
    """Per network shape and (nsub, dt): enable both, init with the edge values, five calls with a new runoff row before each; after
    every call all seven rows against routing.kinematic_call on what the device held before it, bit for bit, and the count.  Asserted
    so that a missing branch cannot hide: a capped and an uncapped positive flow in each of the three stores, QSUR != 0 and QSUB < 0."""
    D = _ctx(base, lib_path, ncells)
    ddist, area, p, volr0, wh0, wt0 = cell_values(ncells, 40 + ncells)
    bytes0 = D.device_bytes
    qs = [set_runoff(D, snwcp(c)) for c in range(3)]  # (three runoff rows serve the five calls in turn)
    hosts = [host_inputs(D, q, area) for q in qs]
    assert ncells < 8 or (qs[0][5] < 0.0 and np.isnan(qs[0][9]))
    seen, widths, qsur_nonzero, qsub_negative = set(), set(), False, False
    cld = (ncells + 63) // 64 * 64
    for name, down in networks(ncells, 50 + ncells).items():
        up = rt.upstream_map(down)
        widths.add(rt.npad_of(up))  # the NPAD the launch picks its kernel by
        for nsub, dt in CASES:
            D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
            bytes1 = D.device_bytes
            D.routing_kinematic_enable(p)
            assert D.device_bytes - bytes1 >= (6 + 7) * 8 * cld
            assert not any(r.any() for r in read_rows(D, ROWS)) and D.routing_count() == 0
            D.routing_init(volr0)
            D.routing_kinematic_init(wh0, wt0)
            wh, wt, volr, qsum = wh0.copy(), wt0.copy(), volr0.copy(), np.zeros(ncells)
            for c in range(5):
                D.upload("qflx_snwcp_liq", snwcp(c % 3))  # the row the call reads is the water balance's of this moment
                D.water_balance(DT)
                D.routing(dt)
                qin, qsur, _ = hosts[c % 3]
                flow_census(seen, wh, wt, volr, area, p, dt / nsub)
                wh, wt, volr, qout = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub)
                with np.errstate(all="ignore"):
                    qsum = rt._canon(qsum + qout)
                    qsur_nonzero |= bool((qsur != 0.0).any())
                    qsub_negative |= bool((qin - qsur < 0.0).any())
                for g, want, what in zip(read_rows(D, ROWS), (volr, qin, qout, qsum, wh, wt, qsur), NAMES):
                    assert bits(g) == bits(want), (name, nsub, dt, c, what, np.nonzero(g.view(np.uint64) != want.view(np.uint64))[0][:5])
                assert D.routing_count() == c + 1
            if ncells > 1:
                assert qin[0] == 0.0 and qsur[0] == 0.0 and not np.signbit(qsur[0])  # the cell without columns
                part = D.routing_read(rt.WT, cell0=ncells // 2, n=ncells - ncells // 2)
                assert bits(part) == bits(wt[ncells // 2:])
            D.routing_clear()  # frees both
            assert D.device_bytes == bytes0
    if ncells >= 63:
        assert seen == {(f, k) for f in ("eh", "et", "er") for k in ("capped", "uncapped")}, seen
        assert qsur_nonzero and qsub_negative
        assert widths == {1, 2, 4, 8}, widths  # every instantiation with_npad can pick
    D.close()


# ---- 2. the edge values, by value ------------------------------------------------------------------------------------------------------
def test_the_edge_values_do_what_the_statement_says(base):
    """The same inputs, looked at by value: a NaN, zero, negative or -inf store releases nothing; +inf releases +inf and leaves NaN
    behind; a capped store releases all it holds in one sub-step; a cell of no area takes no input and its hillslope releases nothing;
    NaN runoff reaches one cell's tributaries and stays there, because a NaN store releases nothing."""
    n, dt = 257, 1800.0
    D = _ctx(base, None, n)
    ddist, area, p, volr0, wh0, wt0 = cell_values(n, 40 + n)
    down = networks(n, 1)["chain"]
    D.routing_enable(down, ddist, area, rt.EFFVEL, 1)
    D.routing_kinematic_enable(p)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    set_runoff(D, snwcp(0))
    D.routing(dt)
    v, qin, qout, _, wh, wt, qsur = read_rows(D, ROWS)
    ch, ct, cr = rt.kinematic_params(p)
    et0 = rt.channel_flow(wt0, p[rt.TLEN], p[rt.TWIDTH], ct, dt)
    er0 = rt.channel_flow(volr0, p[rt.RLEN], p[rt.RWIDTH], cr, dt)
    # VOLR: 0, -0, negative, NaN, -inf release nothing; +inf releases +inf, leaves NaN and hands +inf on
    assert (qout[[1, 3, 5, 11, 15]] == 0.0).all()
    assert qout[13] == INF and np.isnan(v[13]) and v[14] == INF
    assert qout[9] == er0[9] and 1e290 < qout[9] <= 1e300 / dt  # 1e300 m3: the radius is half the width, the rate Manning's or the cap
    assert qout[19] == volr0[19] / dt and qout[20] == volr0[20] / dt  # the cap of the 40 m reaches
    # WH: the same stores release nothing, so each moves by its input alone; +inf leaves NaN and fills the tributaries
    with np.errstate(all="ignore"):
        for c in (24, 26, 28):
            assert wh[c] == wh0[c] + (qsur[c] - 0.0) * dt
        assert np.isnan(wh[34]) and wh[38] == -INF and np.isnan(wh[36]) and wt[36] == INF
        assert wh[32] == 1e300 + (qsur[32] - 1e300 / dt) * dt  # the rate overflows: the cap
    # WT: as VOLR's; the 5 m tributaries release all they hold
    with np.errstate(all="ignore"):
        for c in (41, 43, 45):
            assert wt[c] == wt0[c] + ((rt.hillslope_flow(wh0, area, ch, dt)[c] - 0.0) + (qin[c] - qsur[c])) * dt
    assert np.isnan(wt[51]) and wt[55] == -INF and np.isnan(wt[53]) and v[53] == INF
    assert et0[21] == wt0[21] / dt and et0[22] == wt0[22] / dt
    assert v[21] == volr0[21] + ((er0[20] - er0[21]) + wt0[21] / dt) * dt
    # no area: no input, and the hillslope keeps what it holds
    assert qin[18] == 0.0 and qsur[18] == 0.0 and wh0[18] > 0.0 and wh[18] == wh0[18]
    # the NaN runoff: QIN and QSUB of cell 6 are NaN, its tributaries turn NaN and release nothing from then on
    assert np.isnan(qin[6]) and qin[3] < 0.0 and np.isnan(wt[6]) and np.isfinite(v[6])
    D.routing(dt)
    v2, wt2 = D.routing_read(rt.VOLR), D.routing_read(rt.WT)
    assert np.isnan(wt2[6]) and np.isfinite(v2[6]) and np.isfinite(v2[7]) and np.isfinite(v2[60:]).all() and np.isfinite(wt2[60:]).all()
    D.close()


# ---- the withdrawal with the scheme on ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_withdrawal_on_and_off_with_the_scheme_on(lib_path):
    """K1's "QIN exactly as R1, withdrawal included" (k_kinematic_prep<true>): the irrigation's generated tier stepped until columns
    apply; with the withdrawal on QIN is qin_from_rows with the irrigation's row, QSUR is untouched and QSUB = QIN - QSUR takes the
    withdrawn QIN, all seven rows bit for bit the restatement; off again gives the bits of a context that never called set_withdrawal."""
    n, ncells, nsub = 600, 65, 2
    cols, scal, soil, sched = generated(n, 900)
    rows = prepare(cols, 613)
    ptr, col, w = cell_map(ncells, 8)
    col = (col % n).astype(np.int32)
    ddist, area, p, volr0, wh0, wt0 = cell_values(ncells, 9)
    down = networks(ncells, 10)["forest"]
    up = rt.upstream_map(down)
    ctxs = []
    for k in range(2):
        D = _new(cols, scal, soil, rows, lib_path)
        D.water_balance_enable(TOL)
        D.set_output_grid(ptr, col, w, fill=NAN)
        D.irrigation_enable(sched)
        D.irrigation_init(np.where(sched >= 0, 3.0e-4, 0.0), np.where(np.arange(n) % 3 == 0, 4.0, 0.0))
        D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
        D.routing_kinematic_enable(p)
        D.routing_init(volr0)
        D.routing_kinematic_init(wh0, wt0)
        ctxs.append(D)
    A, B = ctxs  # A never calls set_withdrawal
    B.routing_set_withdrawal(True)
    state = {on: (wh0.copy(), wt0.copy(), volr0.copy(), np.zeros(ncells)) for on in (False, True)}
    differs = False
    for s in range(3):
        for D in ctxs:
            st.kokkos_init_timestep(D)
            D.water_balance_begin()
            st.timestep7_fused(D, DT)
            D.irrigation(DT, 12 * 3600)
            st.kokkos_soil_temperature(D, DT)
            st.kokkos_snow_hydrology(D, DT)
            st.kokkos_surface_fluxes(D, DT)
            D.soil_hydrology(DT)
            D.water_balance(DT)
            D.routing(DT)
        q, qi = B.water_balance_read(hy.WB_QRUNOFF), B.irrigation_read(ir.QFLX_IRRIG)
        surf = (B.soil_hydrology_read(hy.QFLX_SURF), B.soil_hydrology_read(hy.QFLX_H2OSFC_SURF))
        assert (qi > 0.0).any() and bits(q) == bits(A.water_balance_read(hy.WB_QRUNOFF)) and bits(surf[0]) == bits(A.soil_hydrology_read(hy.QFLX_SURF))
        qsur = rt.qsur_from_rows(ptr, col, w, surf[0], surf[1], area)
        for D, on in ((A, False), (B, True)):
            qin = rt.qin_from_rows(ptr, col, w, q, area, qflx_irrig=qi if on else None)
            wh, wt, v, qsum = state[on]
            wh, wt, v, qout = rt.kinematic_call(wh, wt, v, qin, qsur, area, p, up, DT, nsub)
            with np.errstate(all="ignore"):
                qsum = rt._canon(qsum + qout)
            state[on] = (wh, wt, v, qsum)
            for g, want, what in zip(read_rows(D, ROWS), (v, qin, qout, qsum, wh, wt, qsur), NAMES):
                assert bits(g) == bits(want), (s, on, what, np.nonzero(g.view(np.uint64) != want.view(np.uint64))[0][:5])
        differs |= bits(A.routing_read(rt.QIN)) != bits(B.routing_read(rt.QIN))
        assert bits(A.routing_read(rt.QSUR)) == bits(B.routing_read(rt.QSUR))  # the withdrawal takes from QIN, and so from QSUB, alone
    assert differs and bits(state[True][1]) != bits(state[False][1])  # (QSUB feeds the tributaries)
    # off again: from the same storages, the bits of the context that never called it
    B.routing_set_withdrawal(False)
    wh, wt, v, qsum = state[False]
    B.routing_init(v, qsum, A.routing_count())
    B.routing_kinematic_init(wh, wt)
    for D in ctxs:
        D.routing(DT)
    for g, h in zip(read_rows(A, ROWS), read_rows(B, ROWS)):
        assert bits(g) == bits(h)
    for D in ctxs:
        D.close()


# ---- 3. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING


@pytest.fixture(scope="module")
def run_base():
    return rv.run_case()


# (the scheme on the linear routing, the rows left at zero)
_run_context = functools.partial(rv.run_context, parts=("routing", "kinematic"), init=False)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the flag and the scheme on against the stepwise calls in every field and row, then a second run (on
    the captured step when the graph is on) against six more stepwise steps; the host restatement follows the last call's rows."""
    steps = schedule(2 * NSTEPS)
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    assert B.routing_count() == NSTEPS
    a = river_snapshot(A, ROWS)
    assert_same(river_snapshot(B, ROWS), a)
    r = a["route"]
    assert (r[2] > 0.0).any() and (r[4] > 0.0).any() and (r[5] > 0.0).any() and (r[6] != 0.0).any()
    # the next call's rows from the restatement, given the storages before it
    ptr, col, w = run_base["map"]
    area, p = run_base["area"], run_base["p"]
    stepwise(A, run_base["rec"], steps[NSTEPS:NSTEPS + 1], FLAGS)
    qin = rt.qin_from_rows(ptr, col, w, A.water_balance_read(hy.WB_QRUNOFF), area)
    qsur = rt.qsur_from_rows(ptr, col, w, A.soil_hydrology_read(hy.QFLX_SURF), A.soil_hydrology_read(hy.QFLX_H2OSFC_SURF), area)
    wh, wt, v, qout = rt.kinematic_call(r[4], r[5], r[0], qin, qsur, area, p, rt.upstream_map(run_base["down"]), DT, 3)
    for g, want in zip(read_rows(A, (rt.WH, rt.WT, rt.VOLR, rt.QOUT, rt.QSUR)), (wh, wt, v, qout, qsur)):
        assert bits(g) == bits(want)
    stepwise(A, run_base["rec"], steps[NSTEPS + 1:], FLAGS)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(river_snapshot(B, ROWS), river_snapshot(A, ROWS))
    assert B.routing_count() == 2 * NSTEPS
    # the scheme turned off between two runs: the captured step is dropped and the linear scheme runs, as in the stepwise calls
    for X in (A, B):
        X.routing_kinematic_clear()
    stepwise(A, run_base["rec"], steps[:2], FLAGS)
    B.run(DT, steps[:2], FLAGS)
    assert_same(river_snapshot(B, ROWS[:4]), river_snapshot(A, ROWS[:4]))
    assert B.routing_count() == 2 * NSTEPS + 2
    for X in (A, B):
        X.close()


# ---- 4. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it VOLR, QOUT_SUM, the count, WH and WT; a fresh context, restart_load, routing_init,
    routing_kinematic_init, three more steps: the bits of six steps in one context."""
    steps = schedule(NSTEPS)
    A = _run_context(run_base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, ROWS)
    size_a = A.restart_size()
    A.close()
    B = _run_context(run_base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    img, count = B.restart_save(), B.routing_count()
    volr, qsum, wh, wt = read_rows(B, (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT))
    assert count == 3 and B.restart_size() == size_a
    B.close()
    Cx = _run_context(run_base, True, lib_path)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.routing_kinematic_init(wh, wt)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, ROWS), want)
    assert Cx.routing_count() == NSTEPS
    # routing_init leaves WH and WT alone; kinematic_init leaves VOLR, QOUT_SUM and the count alone
    Cx.routing_init(volr, qsum, 2)
    assert bits(Cx.routing_read(rt.WH)) == bits(want["route"][4]) and bits(Cx.routing_read(rt.WT)) == bits(want["route"][5])
    Cx.routing_kinematic_init()
    assert not Cx.routing_read(rt.WH).any() and not Cx.routing_read(rt.WT).any() and not Cx.routing_read(rt.QSUR).any()
    assert bits(Cx.routing_read(rt.VOLR)) == bits(volr) and bits(Cx.routing_read(rt.QOUT_SUM)) == bits(qsum) and Cx.routing_count() == 2
    Cx.close()


# ---- 5. switching schemes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_clear_returns_to_the_linear_scheme(base, lib_path):
    """Three kinematic calls, kinematic_clear, two linear calls: the bits of a context that never had the scheme, given the same VOLR,
    QOUT_SUM and count; and the linear calls are routing.call's."""
    n = 257
    ddist, area, p, volr0, wh0, wt0 = cell_values(n, 40 + n)
    down = networks(n, 50 + n)["forest"]
    A, B = _ctx(base, lib_path, n), _ctx(base, lib_path, n)
    for D in (A, B):
        D.routing_enable(down, ddist, area, rt.EFFVEL, 3)
        set_runoff(D, snwcp(0))
    bytes_linear = A.device_bytes
    A.routing_kinematic_enable(p)
    A.routing_init(volr0)
    A.routing_kinematic_init(wh0, wt0)
    for _ in range(3):
        A.routing(1800.0)
    volr, qsum = A.routing_read(rt.VOLR), A.routing_read(rt.QOUT_SUM)
    assert bits(volr) != bits(volr0)
    A.routing_kinematic_clear()
    A.routing_kinematic_clear()  # nothing to free: OK
    assert A.device_bytes == bytes_linear == B.device_bytes and A.routing_count() == 3
    assert bits(A.routing_read(rt.VOLR)) == bits(volr) and bits(A.routing_read(rt.QOUT_SUM)) == bits(qsum)
    with pytest.raises(L.ElmkError, match="unknown row"):
        A.routing_read(rt.WH)
    B.routing_init(volr, qsum, 3)
    qin = rt.qin_from_rows(*A._map, A.water_balance_read(hy.WB_QRUNOFF), area)
    v = volr
    for _ in range(2):
        for D in (A, B):
            D.routing(1800.0)
        v, qout = rt.call(v, qin, rt.EFFVEL / ddist, rt.upstream_map(down), 1800.0, 3)
    for g, h in zip(read_rows(A, ROWS[:4]), read_rows(B, ROWS[:4])):
        assert bits(g) == bits(h)
    assert bits(A.routing_read(rt.VOLR)) == bits(v) and bits(A.routing_read(rt.QOUT)) == bits(qout) and A.routing_count() == 5
    # ... and on again: the rows come back zero-filled, VOLR stays
    A.routing_kinematic_enable(p)
    assert not A.routing_read(rt.WH).any() and not A.routing_read(rt.WT).any() and bits(A.routing_read(rt.VOLR)) == bits(v)
    A.close()
    B.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(run_base):
    """Every refusal of the four entries, with nothing changed by any; elmk_device_bytes and elmk_restart_size return to their figures
    after the clear.  (The soil hydrology's absence cannot be reached through the entries: the routing needs the water balance, which
    needs it, and its clear is barred while the routing is enabled; the check stands behind them.)"""
    b, rows, m, down, ddist, area, p = (run_base[k] for k in ("b", "rows", "map", "down", "ddist", "area", "p"))
    S1 = schedule(1)

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    D = _run_context(run_base, True, parts=())
    bytes0, size0 = D.device_bytes, D.restart_size()
    before = river_snapshot(D, ())
    refused(lambda: D.routing_kinematic_enable(p), D.routing_kinematic_init, D.routing_kinematic_budget, match="not enabled")
    D.routing_kinematic_clear()  # nothing to free: OK
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(river_snapshot(D, ()), before)
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(np.full(NCELL, 5.0e4))
    bytes1 = D.device_bytes
    state1 = river_snapshot(D, ROWS[:4])
    refused(D.routing_kinematic_init, D.routing_kinematic_budget, match="the scheme is not on")
    refused(lambda: D.routing_read(rt.WH), lambda: D.routing_read(rt.QSUR), match="unknown row")
    for k, name in enumerate(rt.PARAM_NAMES):
        for v in (0.0, -1.0, NAN, INF, -INF):
            q = p.copy()
            q[k, (7 * k) % NCELL] = v
            refused(lambda q=q: D.routing_kinematic_enable(q), match=f"elmk_routing_kinematic_enable: {name} not finite and > 0")
    assert D.lib.elmk_routing_kinematic_enable(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    pc = np.ascontiguousarray(p)
    with captured(D) as cap:
        rc = D.lib.elmk_routing_kinematic_enable(D.ctx, pc.ctypes.data_as(C.c_void_p))
        cap.end()
        assert rc == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS[:4]), state1)

    D.routing_kinematic_enable(p)
    bytes2 = D.device_bytes
    assert bytes2 > bytes1 and D.restart_size() == size0  # the image is what it was
    D.routing_kinematic_init(np.full(NCELL, 2.0e5), np.full(NCELL, 1.0e5))
    state2 = river_snapshot(D, ROWS)
    refused(lambda: D.routing_kinematic_enable(p), match="already on")
    refused(lambda: D.routing_read(7), lambda: D.routing_read(-1), lambda: D.routing_read(rt.WH, cell0=NCELL, n=1))
    for call in (lambda: D.routing_kinematic_init(np.zeros(NCELL + 1)), lambda: D.routing_kinematic_enable(p[:, :-1])):
        with pytest.raises(ValueError):
            call()
    assert D.lib.elmk_routing_kinematic_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap:
        rcs = (D.lib.elmk_routing_kinematic_clear(D.ctx), D.lib.elmk_routing_kinematic_init(D.ctx, None, None))
        cap.end()
        assert rcs == (-1, -1) and b"captured" in D.lib.elmk_last_error(D.ctx)
    refused(D.soil_hydrology_clear, D.water_balance_clear, match="elmk_routing_clear first")
    assert D.device_bytes == bytes2 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS), state2)
    # the following step is the step of a context that met no refusal
    W = _run_context(run_base, True, nsub=2)
    W.routing_init(np.full(NCELL, 5.0e4))
    W.routing_kinematic_init(np.full(NCELL, 2.0e5), np.full(NCELL, 1.0e5))
    for X in (D, W):
        X.run(DT, S1, FLAGS)
    assert_same(river_snapshot(D, ROWS), river_snapshot(W, ROWS))
    D.routing_kinematic_clear()
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    D.routing_kinematic_enable(p)
    D.routing_clear()  # frees both
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    refused(lambda: D.routing_kinematic_enable(p), match="not enabled")
    D.close()
    W.close()


def test_a_context_without_the_scheme_is_what_it_was(run_base):
    """elmk_device_bytes, elmk_restart_size, the image and the routing's rows of a context that never turns the scheme on: the same
    before and after another context of the process has turned it on, run and cleared it, and the same as a fresh context's."""
    steps = schedule(2)
    A = _run_context(run_base, True, parts=("routing",))
    A.run(DT, steps, FLAGS)
    figures = (A.device_bytes, A.restart_size(), bits(A.restart_save()), bits(np.stack(read_rows(A, ROWS[:4]))))
    B = _run_context(run_base, True)
    B.run(DT, steps, FLAGS)
    assert B.device_bytes > figures[0] and B.restart_size() == figures[1]
    assert bits(np.stack(read_rows(B, ROWS[:4]))) != figures[3]  # (the other scheme)
    B.routing_kinematic_clear()
    assert B.device_bytes == figures[0]
    B.close()
    assert (A.device_bytes, A.restart_size(), bits(A.restart_save()), bits(np.stack(read_rows(A, ROWS[:4])))) == figures
    F = _run_context(run_base, True, parts=("routing",))
    F.run(DT, steps, FLAGS)
    assert (F.device_bytes, F.restart_size(), bits(F.restart_save()), bits(np.stack(read_rows(F, ROWS[:4])))) == figures
    A.close()
    F.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_kinematic_routing_demo(tmp_path):
    """examples/kinematic_routing_demo.cc builds with g++ against the C ABI and runs: 48 steps under both schemes, both outlets
    discharge, and the two hydrographs differ."""
    out = run_demo(build_demo("kinematic_routing_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(48))
    lin, kw = np.array([float(s[2]) for s in steps]), np.array([float(s[3]) for s in steps])
    assert lin.max() > 0.0 and kw.max() > 0.0 and (lin >= 0.0).all() and (kw >= 0.0).all() and not np.array_equal(lin, kw)
    assert sum(s.startswith("kinematic:") for s in out) == 2 and sum(s.startswith("linear:") for s in out) == 1


# ---- 7. the budgets ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [1, 65, 1001])
def test_budgets_equal_the_restatements(base, ncells):
    D = _ctx(base, None, ncells)
    ddist, area, p, volr0, wh0, wt0 = cell_values(ncells, 40 + ncells)
    volr0, wh0, wt0 = (np.where(np.isfinite(x) & (x < 1e200), x, 7.0) for x in (volr0, wh0, wt0))
    down = networks(ncells, 5)["forest" if ncells >= 3 else "outlets"]
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_kinematic_enable(p)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    q = snwcp(1)
    q[9] = 2.0e-5
    set_runoff(D, q)
    for _ in range(2):
        D.routing(1800.0)
    v, qin, qout, _, wh, wt, _ = read_rows(D, ROWS)
    want, want_kw = rt.budget(v, qin, qout, down), rt.kinematic_budget(wh, wt)
    assert np.isfinite(want).all() and np.isfinite(want_kw).all() and want[2] > 0.0 and (want_kw > 0.0).all()
    for _ in range(2):  # (in turn: the two share the reduction's scratch)
        assert bits(D.routing_kinematic_budget()) == bits(want_kw)
        assert bits(D.routing_budget()) == bits(want)
    assert bits(D.routing_read(rt.WH)) == bits(wh) and bits(D.routing_read(rt.QOUT)) == bits(qout)  # (the calls change no row)
    D.close()
