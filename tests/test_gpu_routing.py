"""Runoff routing on the device (include/elmk.h "runoff routing"): k_routing against the host restatement (routing.call,
routing.qin_from_rows) bit for bit on every row, in both builds, over ten chained calls on every network shape, size, nsub and dt with
the edge values in cells and columns of their own; the withdrawal on and off; the stage inside elmk_run against the stepwise calls,
graph on and off; restarts through read / count / init; the budget; every refusal and interlock; a context that never enables it."""
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
from tests.river_cases import NCELL, NSTEPS, TOL, read_rows, river_snapshot, set_runoff
from tests.routing_kinematic_cases import cell_map, networks
from tests.run_cases import DT, assert_same, schedule, stepwise
from tests.support import bits, captured

pytestmark = pytest.mark.gpu

NCOLS = 1001
ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM)
NAN, INF = float("nan"), float("inf")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return rv.base()


def runoff(call, lib_path):
    """The column values that become QRUNOFF: the water balance adds qflx_snwcp_liq to the hydrology's runoff terms, which are zero in a
    context whose hydrology has not stepped."""
    rng = np.random.default_rng(700 + call)
    q = rng.uniform(0.0, 4.0e-5, NCOLS)
    q[5], q[9] = -1.0e-5, NAN
    return q


def cell_values(n, seed):
    """ddist, area and the initial VOLR with each edge value in a cell of its own where there are cells enough.  Not
    routing_kinematic_cases.cell_values: that one draws the scheme's parameters before VOLR and has no capped reaches (ddist 19 .. 21)."""
    rng = np.random.default_rng(seed)
    ddist = np.exp(rng.uniform(np.log(500.0), np.log(60000.0), n))
    area = rng.uniform(0.5e8, 2.5e8, n)
    volr = rng.uniform(0.0, 1.0e6, n)
    special = [0.0, -0.0, -3.5e4, 5e-324, 1e300, NAN, INF, -INF]
    for i, v in enumerate(special):
        if 2 * i + 1 < n:
            volr[2 * i + 1] = v
    if n > 20:
        area[18] = 0.0
        ddist[19] = ddist[20] = 40.0  # the cap at every dt and nsub of the test but 1 s
        ddist[21 % n] = 1.0e-3        # ... and there too
    return ddist, area, volr


NSUBS, DTS = (1, 2, 7, 64), (1.0, 1800.0, 86400.0)


_ctx = functools.partial(rv.context, hydrology=False)  # (the hydrology has not stepped: its runoff terms are zero)


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 257, 1001])
def test_ten_chained_calls_equal_the_restatement(base, ncells, lib_path):
    """Per network shape, nsub and dt: enable, init with the edge
    values, ten calls with a new runoff row before each; after every call VOLR, QIN, QOUT and QOUT_SUM against routing.call on what the
    device held before it, bit for bit, and the count."""
    D = _ctx(base, lib_path, ncells)
    ptr, col, w = D._map
    ddist, area, volr0 = cell_values(ncells, 40 + ncells)
    kout = rt.EFFVEL / ddist
    bytes0 = D.device_bytes
    qs = [set_runoff(D, runoff(c, lib_path)) for c in range(3)]  # (three runoff rows serve the ten calls in turn)
    assert ncells < 8 or (qs[0][5] < 0.0 and np.isnan(qs[0][9]))
    seen, widths = set(), set()
    for name, down in networks(ncells, 50 + ncells).items():
        up = rt.upstream_map(down)
        widths.add(rt.npad_of(up))  # the NPAD the launch picks its kernel by
        for nsub, dt in ((n_, d_) for n_ in NSUBS for d_ in DTS):
            seen.add((nsub, dt))
            D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
            cld = (ncells + 63) // 64 * 64
            npad = rt.npad_of(up)
            assert D.device_bytes - bytes0 >= (6 * 8 + 8 + 8 + 4 * npad + 4) * cld
            assert not any(r.any() for r in read_rows(D, ROWS)) and D.routing_count() == 0
            D.routing_init(volr0)
            volr, qsum = volr0.copy(), np.zeros(ncells)
            for c in range(10):
                q = qs[c % 3]
                D.upload("qflx_snwcp_liq", q)  # the row the call reads is the water balance's of this moment
                D.water_balance(DT)
                D.routing(dt)
                qin = rt.qin_from_rows(ptr, col, w, q, area)
                volr, qout = rt.call(volr, qin, kout, up, dt, nsub)
                with np.errstate(all="ignore"):
                    qsum = rt._canon(qsum + qout)
                got = read_rows(D, ROWS)
                for g, want, what in zip(got, (volr, qin, qout, qsum), ("VOLR", "QIN", "QOUT", "QOUT_SUM")):
                    assert bits(g) == bits(want), (name, nsub, dt, c, what, np.nonzero(g.view(np.uint64) != want.view(np.uint64))[0][:5])
                assert D.routing_count() == c + 1
            if ncells > 1:
                assert qin[0] == 0.0 and not np.signbit(qin[0])  # the cell without columns
                part = D.routing_read(rt.VOLR, cell0=ncells // 2, n=ncells - ncells // 2)
                assert bits(part) == bits(volr[ncells // 2:])
            D.routing_clear()
            assert D.device_bytes == bytes0
    assert seen == {(n, d) for n in NSUBS for d in DTS}
    if ncells >= 63:
        assert widths == {1, 2, 4, 8}, widths  # every instantiation with_npad can pick
    D.close()


def test_the_edge_values_do_what_the_statement_says(base):
    """The same inputs, looked at by value: a NaN, zero, negative or -inf storage releases nothing; +inf releases +inf and leaves NaN
    behind; a capped cell releases all it holds in one sub-step; a cell of no area takes no input; NaN runoff reaches one cell and
    stays there, because a NaN storage releases nothing."""
    n = 257
    D = _ctx(base, None, n)
    ddist, area, volr0 = cell_values(n, 40 + n)
    down = networks(n, 1)["chain"]
    D.routing_enable(down, ddist, area, rt.EFFVEL, 1)
    D.routing_init(volr0)
    set_runoff(D, runoff(0, None))
    D.routing(1800.0)
    v, qin, qout, _ = read_rows(D, ROWS)
    assert (qout[[1, 3, 5, 11, 15]] == 0.0).all()  # 0, -0, negative, NaN, -inf
    assert qout[13] == INF and np.isnan(v[13]) and v[14] == INF
    assert qout[9] == rt.flow(np.array([1e300]), rt.EFFVEL / ddist[9], 1800.0)[0] and qout[9] > 1e290
    assert qin[18] == 0.0 and np.isnan(qin[6]) and qin[3] < 0.0 and np.isnan(v[6])
    assert qout[19] == volr0[19] / 1800.0 and qout[20] == volr0[20] / 1800.0  # the cap
    D.routing(1800.0)
    v2 = D.routing_read(rt.VOLR)
    assert np.isnan(v2[6]) and np.isfinite(v2[7]) and np.isfinite(v2[30:]).all()  # (a NaN storage releases nothing: it stays where it is)
    D.close()


# ---- 2. the withdrawal ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_withdrawal_on_and_off(lib_path):
    """The irrigation's generated tier: the seven wrappers and the stage until columns apply; then routing with the withdrawal on
    subtracts the aggregate of QFLX_IRRIG, bit for bit the restatement, drives some cells' storage negative, and those release nothing;
    off again gives the bits of a context that never called set_withdrawal."""
    n, ncells = 600, 65
    cols, scal, soil, sched = generated(n, 900)
    rows = prepare(cols, 613)
    ptr, col, w = cell_map(ncells, 8)
    col = (col % n).astype(np.int32)
    ddist, area, _ = cell_values(ncells, 9)
    down = networks(ncells, 10)["forest"]
    up, kout = rt.upstream_map(down), rt.EFFVEL / ddist
    ctxs = []
    for k in range(2):
        D = _new(cols, scal, soil, rows, lib_path)
        D.water_balance_enable(TOL)
        D.set_output_grid(ptr, col, w, fill=NAN)
        D.irrigation_enable(sched)
        D.irrigation_init(np.where(sched >= 0, 3.0e-4, 0.0), np.where(np.arange(n) % 3 == 0, 4.0, 0.0))
        D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
        ctxs.append(D)
    A, B = ctxs  # A never calls set_withdrawal
    B.routing_set_withdrawal(True)
    with pytest.raises(L.ElmkError, match="elmk_routing_clear first"):
        B.irrigation_clear()
    volr = {True: np.zeros(ncells), False: np.zeros(ncells)}
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
        assert (qi > 0.0).any() and bits(q) == bits(A.water_balance_read(hy.WB_QRUNOFF))
        for D, on in ((A, False), (B, True)):
            qin = rt.qin_from_rows(ptr, col, w, q, area, qflx_irrig=qi if on else None)
            volr[on], qout = rt.call(volr[on], qin, kout, up, DT, 2)
            got = read_rows(D, ROWS)
            assert bits(got[0]) == bits(volr[on]) and bits(got[1]) == bits(qin) and bits(got[2]) == bits(qout), (s, on)
    assert (volr[True] < 0.0).any() and bits(volr[True]) != bits(volr[False])
    assert (B.routing_read(rt.QOUT)[volr[True] < 0.0] >= 0.0).all()
    # off again: from the same storages, the bits of the context that never called it
    B.routing_set_withdrawal(False)
    B.irrigation_clear()  # (no longer barred)
    B.routing_init(volr[False], A.routing_read(rt.QOUT_SUM), A.routing_count())
    for D in ctxs:
        D.routing(DT)
    for g, h in zip(read_rows(A, ROWS), read_rows(B, ROWS)):
        assert bits(g) == bits(h)
    with pytest.raises(L.ElmkError, match="irrigation is not enabled"):
        B.routing_set_withdrawal(True)
    for D in ctxs:
        D.close()


# ---- 3. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING


@pytest.fixture(scope="module")
def run_base():
    G = rv.run_case()
    G["ddist"] = cell_values(NCELL, 78)[0]  # (this module's cell_values: with the capped cells' short reaches)
    return G


# (the linear scheme alone, its rows left at zero)
_run_context = functools.partial(rv.run_context, parts=("routing",), init=False)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the flag against the stepwise calls in every field and row, then a second run (on the captured step
    when the graph is on) against six more stepwise steps; the host restatement follows the same rows; the count advances by nsteps."""
    steps = schedule(2 * NSTEPS)
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    assert B.routing_count() == NSTEPS
    a = river_snapshot(A, ROWS)
    assert_same(river_snapshot(B, ROWS), a)
    assert (a["route"][rt.QOUT] > 0.0).any() and (a["wb"][hy.WB_QRUNOFF] != 0.0).any()
    # the last call's rows from the restatement, given the storages before it
    ptr, col, w = run_base["map"]
    stepwise(A, run_base["rec"], steps[NSTEPS:NSTEPS + 1], FLAGS)
    qin = rt.qin_from_rows(ptr, col, w, A.water_balance_read(hy.WB_QRUNOFF), run_base["area"])
    v, qout = rt.call(a["route"][rt.VOLR], qin, rt.EFFVEL / run_base["ddist"], rt.upstream_map(run_base["down"]), DT, 3)
    assert bits(A.routing_read(rt.VOLR)) == bits(v) and bits(A.routing_read(rt.QOUT)) == bits(qout)
    stepwise(A, run_base["rec"], steps[NSTEPS + 1:], FLAGS)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(river_snapshot(B, ROWS), river_snapshot(A, ROWS))
    assert B.routing_count() == 2 * NSTEPS
    # without the flag the rows stay put, and the run is the run of a context without the feature
    P = _run_context(run_base, graph, parts=())
    P.run(DT, steps[:NSTEPS], FLAGS & ~st.RUN_ROUTING)
    P.run(DT, steps[NSTEPS:], FLAGS & ~st.RUN_ROUTING)
    before = np.stack(read_rows(B, ROWS))
    B2 = _run_context(run_base, graph)
    B2.run(DT, steps[:NSTEPS], FLAGS & ~st.RUN_ROUTING)
    B2.run(DT, steps[NSTEPS:], FLAGS & ~st.RUN_ROUTING)
    assert not np.stack(read_rows(B2, ROWS)).any() and B2.routing_count() == 0
    assert_same(river_snapshot(B2, ()), river_snapshot(P, ()))
    assert_same(river_snapshot(B, ()), river_snapshot(P, ()))
    assert bits(np.stack(read_rows(B, ROWS))) == bits(before)
    for D in (A, B, B2, P):
        D.close()


# ---- 4. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it VOLR, QOUT_SUM and the count; a fresh context, restart_load, routing_init, three more
    steps: the bits of six steps in one context, and the same mean discharge QOUT_SUM / count."""
    steps = schedule(NSTEPS)
    A = _run_context(run_base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, ROWS)
    size_a = A.restart_size()
    A.close()
    B = _run_context(run_base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    img, volr, qsum, count = B.restart_save(), B.routing_read(rt.VOLR), B.routing_read(rt.QOUT_SUM), B.routing_count()
    assert count == 3 and B.restart_size() == size_a
    B.close()
    Cx = _run_context(run_base, True, lib_path)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.run(DT, steps[3:], FLAGS)
    got = river_snapshot(Cx, ROWS)
    assert_same(got, want)
    assert Cx.routing_count() == NSTEPS
    with np.errstate(all="ignore"):
        assert bits(got["route"][rt.QOUT_SUM] / Cx.routing_count()) == bits(want["route"][rt.QOUT_SUM] / NSTEPS)
    # the mean's reset
    Cx.routing_reset_mean()
    assert Cx.routing_count() == 0 and not Cx.routing_read(rt.QOUT_SUM).any() and bits(Cx.routing_read(rt.VOLR)) == bits(want["route"][rt.VOLR])
    Cx.close()


# ---- 5. the budget -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [1, 65, 1001])
def test_budget_equals_the_restatement(base, ncells):
    D = _ctx(base, None, ncells)
    ddist, area, volr0 = cell_values(ncells, 40 + ncells)
    volr0 = np.where(np.isfinite(volr0), volr0, 7.0)
    down = networks(ncells, 5)["forest" if ncells >= 3 else "outlets"]
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr0)
    q = runoff(1, None)
    q[9] = 2.0e-5
    set_runoff(D, q)
    for _ in range(2):
        D.routing(1800.0)
    v, qin, qout, _ = read_rows(D, ROWS)
    got, want = D.routing_budget(), rt.budget(v, qin, qout, down)
    assert np.isfinite(want).all() and want[2] > 0.0
    assert bits(got) == bits(want)
    assert bits(D.routing_budget()) == bits(want) and bits(D.routing_read(rt.QOUT)) == bits(qout)  # (the call changes no row)
    D.close()


# ---- 6. refusals and interlocks ------------------------------------------------------------------------------------------------------
def test_refusals_and_interlocks_change_nothing(run_base):
    b, rows, m, down, ddist, area = (run_base[k] for k in ("b", "rows", "map", "down", "ddist", "area"))
    S1 = schedule(1)

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    D = _run_context(run_base, True, parts=())
    bytes0, size0 = D.device_bytes, D.restart_size()
    before = river_snapshot(D, ())
    refused(lambda: D.routing(DT), D.routing_init, lambda: D.routing_read(0), D.routing_count, D.routing_reset_mean, D.routing_budget,
            lambda: D.routing_set_withdrawal(True), match="not enabled")
    refused(lambda: D.run(DT, S1, FLAGS), match="without the runoff routing enabled")
    bad = lambda i, v: np.where(np.arange(NCELL) == i, v, down).astype(np.int32)  # noqa: E731
    vec = lambda a, i, v: np.where(np.arange(NCELL) == i, v, a)  # noqa: E731
    two_cycle = down.copy()
    j = int(np.nonzero(down >= 0)[0][0])
    two_cycle[down[j]] = j
    nine = np.zeros(NCELL, np.int32)
    nine[0], nine[10:] = -1, -1
    refused(lambda: D.routing_enable(down[:-1], ddist[:-1], area[:-1]), match="ncells differs")
    refused(lambda: D.routing_enable(bad(4, -2), ddist, area), lambda: D.routing_enable(bad(4, NCELL), ddist, area), match="down outside")
    refused(lambda: D.routing_enable(bad(4, 4), ddist, area), match="its own index")
    refused(lambda: D.routing_enable(two_cycle, ddist, area), match="cycle")
    refused(lambda: D.routing_enable(nine, ddist, area), match="more than 8")
    refused(*(lambda v=v: D.routing_enable(down, vec(ddist, 7, v), area) for v in (0.0, -1.0, NAN, INF)), match="ddist")
    refused(*(lambda v=v: D.routing_enable(down, ddist, vec(area, 7, v)) for v in (-1.0, NAN, INF)), match="area")
    refused(*(lambda v=v: D.routing_enable(down, ddist, area, v) for v in (0.0, -0.35, NAN, INF)), match="effvel")
    refused(*(lambda v=v: D.routing_enable(down, ddist, area, 0.35, v) for v in (0, -1, 65)), match="nsub")
    P = C.c_void_p
    d32, dd, aa = np.ascontiguousarray(down, np.int32), np.ascontiguousarray(ddist), np.ascontiguousarray(area)
    ptrs = [x.ctypes.data_as(P) for x in (d32, dd, aa)]
    for k in range(3):
        args = list(ptrs)
        args[k] = None
        assert D.lib.elmk_routing_enable(D.ctx, NCELL, *args, 0.35, 1) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    # a stream being captured
    with captured(D) as cap:
        rc = D.lib.elmk_routing_enable(D.ctx, NCELL, *ptrs, 0.35, 1)
        cap.end()
        assert rc == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    D.routing_clear()  # nothing to free: OK
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(river_snapshot(D, ()), before)
    # what the feature needs
    N = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    refused(lambda: N.routing_enable(down, ddist, area), match="no output grid")
    N.set_output_grid(*m, fill=NAN)
    refused(lambda: N.routing_enable(down, ddist, area), match="water balance is not enabled")
    N.close()

    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    bytes1 = D.device_bytes
    assert D.restart_size() == size0  # the image is what it was
    D.routing_init(np.full(NCELL, 5.0e4))
    state1 = river_snapshot(D, ROWS)
    refused(lambda: D.routing_enable(down, ddist, area), match="already enabled")
    refused(*(lambda dt=dt: D.routing(dt) for dt in (0.0, -1800.0, NAN, INF)), match="dt must be finite and positive")
    refused(lambda: D.routing_read(4), lambda: D.routing_read(-1), lambda: D.routing_read(0, cell0=NCELL, n=1),
            lambda: D.routing_read(0, cell0=NCELL - 1, n=2), lambda: D.routing_read(0, cell0=-1, n=1), lambda: D.routing_init(ncalls=-1),
            lambda: D.run(DT, S1, FLAGS & ~st.RUN_WATER_BALANCE), lambda: D.routing_set_withdrawal(True))
    refused(lambda: D.set_output_grid(*m, fill=0.0), D.clear_output_grid, D.water_balance_clear, D.soil_hydrology_clear,
            match="elmk_routing_clear first")
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS), state1)
    # the following step is the step of a context that met no refusal
    W = _run_context(run_base, True, nsub=2)
    W.routing_init(np.full(NCELL, 5.0e4))
    for X in (D, W):
        X.run(DT, S1, FLAGS)
    assert_same(river_snapshot(D, ROWS), river_snapshot(W, ROWS))
    D.routing_clear()
    refused(lambda: D.routing_read(0), match="not enabled")
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    D.water_balance_clear()  # (no longer barred)
    D.close()
    W.close()


# ---- 7. a context that never enables the feature ------------------------------------------------------------------------------------
def test_a_context_without_the_feature_is_what_it_was(run_base):
    """elmk_device_bytes, elmk_restart_size and the image of a context that never enables the feature: the same before and after another
    context of the process has enabled, run and cleared it, the same as a fresh context's afterwards, and the same through an enable
    and a clear of its own."""
    steps = schedule(2)
    A = _run_context(run_base, True, parts=())
    A.run(DT, steps, FLAGS & ~st.RUN_ROUTING)
    figures = (A.device_bytes, A.restart_size(), bits(A.restart_save()))
    B = _run_context(run_base, True)
    B.run(DT, steps, FLAGS)
    assert B.device_bytes > figures[0] and B.restart_size() == figures[1]
    B.routing_clear()
    assert B.device_bytes == figures[0]
    B.close()
    assert (A.device_bytes, A.restart_size(), bits(A.restart_save())) == figures
    F = _run_context(run_base, True, parts=())
    F.run(DT, steps, FLAGS & ~st.RUN_ROUTING)
    assert (F.device_bytes, F.restart_size(), bits(F.restart_save())) == figures
    F.routing_enable(run_base["down"], run_base["ddist"], run_base["area"])
    F.routing_clear()
    assert (F.device_bytes, F.restart_size(), bits(F.restart_save())) == figures
    A.close()
    F.close()
