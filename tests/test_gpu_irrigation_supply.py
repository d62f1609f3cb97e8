"""The irrigation's river supply limit on the device (include/elmk.h "irrigation: river supply limit"): k_irrigation_supply against the
host restatement (irrigation.supply_limit) bit for bit in both builds over ten chained steps that hold every case of the statement; the
limit inside elmk_run against the stepwise calls, graph on and off, switched off and on again between runs; 3 + 3 steps through the
image and the read / init pairs; every refusal and interlock; the figures of a context that never enables the limit; the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests.hydrology_cases import _new, clear_snow, prepare
from tests.irrigation_cases import generated, smpso_of
from tests.irrigation_supply_cases import CASES, INF, NAN, cell_map, cell_values, census
from tests.run_cases import DT, NREC, SERIES, _inputs, assert_same, same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

TOL = 1.0e-9
SUP = (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)


def _sup_rows(D):
    return np.stack([D.irrigation_supply_read(w) for w in SUP])


def _enable_all(D, m, sched, down, ddist, area, nsub=1, thr=None):
    """The output grid, the irrigation, the routing with the withdrawal on and, with thr, the limit; the limit's rows are counted."""
    D.set_output_grid(*m, fill=NAN)
    D.irrigation_enable(sched)
    D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
    D.routing_set_withdrawal(True)
    if thr is not None:
        before = D.device_bytes
        D.irrigation_supply_enable(thr)
        assert D.device_bytes - before == 4 * 8 * ((len(area) + 63) // 64 * 64)
    return D


# ---- 1. the kernel against the restatement -------------------------------------------------------------------------------------------
N1, NCELL1 = 5003, 70


@pytest.mark.parametrize("thr", [0.0, 0.1])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_ten_chained_steps_equal_the_restatement(lib_path, thr):
    """5003 columns (no multiple of 64) of the irrigation's generated tier over 70 cells (two workgroups of 64 cells, the second with
    six): cell 3 holds 2100 columns, more than two LDS tiles; cells 0 and 61 .. 66 are empty, a run across the workgroup boundary;
    cells 5 and 7 hold one column; fifty columns lie in no cell.  Ten steps of the seven wrappers and elmk_irrigation with the limit
    behind it, from rows in which windows are open already: after every step RATE and the four cell rows against irrigation.step
    followed by irrigation.supply_limit, bit for bit, NLEFT and QFLX_IRRIG as the irrigation alone leaves them.  RATE, NLEFT and
    UNMET_SUM chain; VOLR is set before every step (elmk_routing_init), with the edge storages in cells 8 .. 13 and the others drawn
    anew, so that over the ten steps every case of the host test's list is met."""
    cols, scal, soil, sched = generated(N1, 900)
    rows0 = prepare(cols, 614)
    m = cell_map(N1, NCELL1, 51, big=(3, 2100), empty=(0, 61, 62, 63, 64, 65, 66), single=(5, 7), free=50)
    ptr, col, w = m
    assert np.unique(col).size == col.size and int(np.diff(ptr).max()) > 2048
    area, _ = cell_values(NCELL1, 52)
    D = _new(cols, scal, soil, rows0, lib_path)
    D.water_balance_enable(TOL)
    _enable_all(D, m, sched, np.full(NCELL1, -1, np.int32), np.full(NCELL1, 5.0e4), area, thr=thr)
    c = np.arange(N1)
    D.irrigation_init(np.where(sched >= 0, 1.0e-4 + 1.0e-6 * (c % 97), 0.0), np.where(c % 3 == 0, (c % 7).astype(np.float64), 0.0))
    smpso = smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    rows, unmet = D.irrigation_rows(), np.zeros(NCELL1)
    seen = dict.fromkeys(CASES, 0)
    limited = 0
    for s in range(10):
        tod = (5 * 3600 + 1800 * s) % 86400
        _, volr = cell_values(NCELL1, 60 + s, lo=2.0 + 0.3 * s, hi=7.0)
        D.routing_init(volr)
        st.timestep7_fused(D, DT)
        fields = {k: D[k] for k in ir.READS}
        _, want = ir.step(fields, rows, sched, DT, tod, smpso, stored=stored)
        want_rate, want_sup = ir.supply_limit(ptr, col, w, area, volr, want[ir.RATE], want[ir.NLEFT], int(DT), thr, unmet,
                                              qflx_irrig=want[ir.QFLX_IRRIG])
        D.irrigation(DT, tod)
        rows, sup = D.irrigation_rows(), _sup_rows(D)
        assert bits(rows[ir.RATE]) == bits(want_rate), (s, "RATE", np.nonzero(rows[ir.RATE] != want_rate)[0][:5])
        assert bits(rows[ir.NLEFT]) == bits(want[ir.NLEFT]) and bits(rows[ir.QFLX_IRRIG]) == bits(want[ir.QFLX_IRRIG]), s
        for k in SUP:
            assert bits(sup[k]) == bits(want_sup[k]), (s, "row", k, np.nonzero(sup[k] != want_sup[k])[0][:5])
        assert bits(D.routing_read(rt.VOLR)) == bits(volr)  # (the limit only reads it)
        for k, v in census(ptr, col, N1, volr, want[ir.NLEFT], want[ir.RATE], 8, want_sup).items():
            seen[k] += v
        limited += int((rows[ir.RATE] != want[ir.RATE]).sum())
        unmet = sup[ir.UNMET_SUM]
    print("census over ten steps:", seen, "columns cut back:", limited)
    assert all(seen[k] > 0 for k in CASES), [k for k in CASES if not seen[k]]
    assert limited > 0
    part = D.irrigation_supply_read(ir.UNMET_SUM, cell0=33, n=NCELL1 - 33)
    assert bits(part) == bits(unmet[33:])
    D.irrigation_supply_reset()
    assert not D.irrigation_supply_read(ir.UNMET_SUM).any() and bits(D.irrigation_supply_read(ir.DEMAND)) == bits(sup[ir.DEMAND])
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------
NCOL, NCELL, NSTEPS = 193, 70, 6
FLAGS = st.RUN_IRRIGATION | st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING
THR = 0.1


@pytest.fixture(scope="module")
def base():
    b = _inputs(NCOL, 531)
    cols = b[0]
    clear_snow(cols)
    rows = prepare(cols, 532)
    c = np.arange(NCOL)
    cols["t_soisno"][:, 5:] = np.maximum(cols["t_soisno"][:, 5:], 276.0)
    # schedule() starts at 21:00 UTC: column c passes 06:00 local in step c % 6 of a run, or (one in seven) is not irrigated
    sched = ((32400 - 1800 * (c % 6) + 100 * (c % 5)) % 86400).astype(np.int32)
    sched[c % 7 == 3] = -1
    m = cell_map(NCOL, NCELL, 71, empty=(0, 63, 64), single=(5,), free=3)
    rng = np.random.default_rng(72)
    down = np.full(NCELL, -1, np.int32)
    down[1:40] = np.arange(2, 41) % NCELL  # a chain through cells 1 .. 40, the rest outlets
    down[40] = -1
    ddist = np.exp(rng.uniform(np.log(500.0), np.log(60000.0), NCELL))
    area, _ = cell_values(NCELL, 73)
    volr0 = 10.0 ** rng.uniform(1.0, 6.0, NCELL)
    return b, rows, sched, m, down, ddist, area, volr0


def _context(base, graph, lib_path=None, thr=THR):
    b, rows, sched, m, down, ddist, area, volr0 = base
    D = _new(b[0], b[1], b[2], rows, lib_path, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    _enable_all(D, m, sched, down, ddist, area, nsub=2, thr=thr)
    D.routing_init(volr0)
    return D


def _snapshot(D, limit=True):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out["hyd"], out["wb"], out["irr"] = D.soil_hydrology_rows(), D.water_balance_rows(), D.irrigation_rows()
    out["route"] = np.stack([D.routing_read(w) for w in range(4)])
    if limit:
        out["sup"] = _sup_rows(D)
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise_and_the_key_follows_the_switch(base, graph):
    """Six steps of elmk_run with the four flags against the stepwise calls in every field and row, the limit on; then the limit
    cleared in both and six more steps (with the graph on the step is captured anew: the captured one had the limiter's node); then on
    again, UNMET_SUM carried over through read / init, and the first six steps' schedule once more.  The limit changes what the run
    computes: a context with the limit off from the start ends with other rates and other storages."""
    steps = schedule(2 * NSTEPS)
    rec = base[0][5]
    A, B = _context(base, False), _context(base, graph)
    stepwise(A, rec, steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["sup"][ir.UNMET_SUM] > 0.0).any() and (a["irr"][ir.NLEFT] > 0.0).any()
    P = _context(base, graph, thr=None)  # never limited
    P.run(DT, steps[:NSTEPS], FLAGS)
    p = _snapshot(P, limit=False)
    assert not same(p["irr"][ir.RATE], a["irr"][ir.RATE]) and not same(p["route"][rt.VOLR], a["route"][rt.VOLR])
    assert (p["irr"][ir.RATE] >= a["irr"][ir.RATE]).all()
    # off
    unmet = a["sup"][ir.UNMET_SUM]
    for D in (A, B):
        D.irrigation_supply_clear()
    stepwise(A, rec, steps[NSTEPS:], FLAGS)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(_snapshot(B, limit=False), _snapshot(A, limit=False))
    # on again
    for D in (A, B):
        D.irrigation_supply_enable(THR)
        D.irrigation_supply_init(unmet)
    stepwise(A, rec, steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["sup"][ir.UNMET_SUM] >= unmet).all()
    for D in (A, B, P):
        D.close()


# ---- 3. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(base, lib_path):
    """Three steps, the column image (version 5: it carries RATE and NLEFT) and beside it VOLR, QOUT_SUM, the count and UNMET_SUM; a
    fresh context, restart_load, routing_init, irrigation_supply_init, three more steps: the bits of six steps in one context.  The
    image is the image of a context without the limit, byte for byte in size."""
    steps = schedule(NSTEPS)
    A = _context(base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want, size_a = _snapshot(A), A.restart_size()
    A.close()
    B = _context(base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    assert (B.irrigation_read(ir.NLEFT) > 0.0).any()
    img, volr, qsum, count = B.restart_save(), B.routing_read(rt.VOLR), B.routing_read(rt.QOUT_SUM), B.routing_count()
    unmet = B.irrigation_supply_read(ir.UNMET_SUM)
    assert B.restart_size() == size_a
    B.irrigation_supply_clear()
    assert B.restart_size() == size_a
    B.close()
    Cx = _context(base, True, lib_path)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.irrigation_supply_init(unmet)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(_snapshot(Cx), want)
    Cx.close()


# ---- 4. refusals and interlocks ------------------------------------------------------------------------------------------------------
def test_refusals_and_interlocks_change_nothing(base):
    b, rows, sched, m, down, ddist, area, volr0 = base
    S1 = schedule(1)

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    # what the limit needs, in the order it asks
    D = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    D.set_graph(True)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    refused(lambda: D.irrigation_supply_enable(THR), match="irrigation is not enabled")
    refused(D.irrigation_supply_init, lambda: D.irrigation_supply_read(0, n=1), D.irrigation_supply_reset, match="not enabled")
    D.irrigation_supply_clear()  # nothing to free: OK
    shared = (m[0], np.where(np.arange(m[1].size) == 40, m[1][7], m[1]).astype(np.int32), m[2])  # term 40 repeats term 7's column
    D.set_output_grid(*shared, fill=NAN)
    D.irrigation_enable(sched)
    refused(lambda: D.irrigation_supply_enable(THR), match="routing is not enabled")
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr0)
    refused(lambda: D.irrigation_supply_enable(THR), match="withdrawal is off")
    D.routing_set_withdrawal(True)
    bytes0, size0 = D.device_bytes, D.restart_size()
    before = _snapshot(D, limit=False)
    refused(*(lambda v=v: D.irrigation_supply_enable(v) for v in (-0.1, 1.0, 1.5, NAN, INF, -INF)), match="threshold")
    refused(lambda: D.irrigation_supply_enable(THR), match=f"column {int(m[1][7])} is in more than one cell")
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(_snapshot(D, limit=False), before)
    # the map the tests use: every column once
    D.routing_set_withdrawal(False)
    D.routing_clear()
    D.set_output_grid(*m, fill=NAN)
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr0)
    D.routing_set_withdrawal(True)
    bytes0 = D.device_bytes
    # a stream being captured
    with captured(D) as cap:
        rc = D.lib.elmk_irrigation_supply_enable(D.ctx, C.c_double(THR))
        cap.end()
        assert rc == -1 and b"captured" in D.lib.elmk_last_error(D.ctx) and D.device_bytes == bytes0
    D.irrigation_supply_enable(THR)
    bytes1 = D.device_bytes
    assert bytes1 - bytes0 == 4 * 8 * 128 and D.restart_size() == size0
    D.irrigation_supply_init(np.full(NCELL, 7.0))
    state1 = _snapshot(D)
    refused(lambda: D.irrigation_supply_enable(THR), match="already enabled")
    refused(lambda: D.irrigation_supply_read(4), lambda: D.irrigation_supply_read(-1), lambda: D.irrigation_supply_read(0, cell0=NCELL, n=1),
            lambda: D.irrigation_supply_read(0, cell0=NCELL - 1, n=2), lambda: D.irrigation_supply_read(0, cell0=-1, n=1))
    # what the limit reads stays
    refused(lambda: D.routing_set_withdrawal(False), D.routing_clear, D.irrigation_clear, lambda: D.set_output_grid(*m, fill=0.0),
            D.clear_output_grid, match="elmk_irrigation_supply_clear first")
    # the kinematic-wave scheme keeps VOLR's buffer where it is: on and off stay allowed, and change nothing the limit reads
    params = np.full((st.ROUTE_KW_NPARAM, NCELL), 1.0)
    D.routing_kinematic_enable(params)
    D.routing_kinematic_clear()
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(_snapshot(D), state1)
    # the following step is the step of a context that met no refusal
    W = _context(base, True)
    W.irrigation_supply_init(np.full(NCELL, 7.0))
    for X in (D, W):
        X.run(DT, S1, FLAGS)
    assert_same(_snapshot(D), _snapshot(W))
    # the clear: the figures from before the enable, the existing refusals in their old words
    D.irrigation_supply_clear()
    refused(lambda: D.irrigation_supply_read(0), match="not enabled")
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    refused(D.irrigation_clear, lambda: D.set_output_grid(*m, fill=0.0), D.clear_output_grid, match="elmk_routing_clear first")
    D.routing_set_withdrawal(False)  # (no longer barred)
    D.close()
    W.close()


# ---- 5. a context that never enables the limit ---------------------------------------------------------------------------------------
def test_a_context_without_the_limit_is_what_it_was(base):
    """A context with the irrigation and the routing that never enables the limit, one that enables and clears it before it runs, and
    the host restatement of the irrigation without the limit: the same bits in every field and row, the same elmk_device_bytes,
    elmk_restart_size and image; RATE is irrigation.step's, never cut back."""
    steps = schedule(3)
    A, B = _context(base, True, thr=None), _context(base, True, thr=None)
    figures = (A.device_bytes, A.restart_size())
    B.irrigation_supply_enable(THR)
    assert B.device_bytes > figures[0] and B.restart_size() == figures[1]
    B.irrigation_supply_clear()
    assert (B.device_bytes, B.restart_size()) == figures
    for D in (A, B):
        D.run(DT, steps, FLAGS)
    assert_same(_snapshot(A, limit=False), _snapshot(B, limit=False))
    assert bits(A.restart_save()) == bits(B.restart_save()) and (A.device_bytes, A.restart_size()) == (B.device_bytes, B.restart_size())
    # the step after, stepwise, against irrigation.step alone
    p = schedule(4)[3:]
    rows = A.irrigation_rows()
    A.solar_geometry(DT, float(p[0]["decday"]), int(p[0]["doy"]))
    st.timestep7_fused(A, DT)
    fields = {k: A[k] for k in ir.READS}
    tod = ir.time_of_day(float(p[0]["decday"]), int(p[0]["doy"]))
    _, want = ir.step(fields, rows, base[2], DT, tod, smpso_of(base[0][0]["vtype"]))
    A.irrigation(DT, tod)
    assert bits(A.irrigation_rows()) == bits(want)
    A.close()
    B.close()


# ---- 6. the demo --------------------------------------------------------------------------------------------------------------------
def test_irrigation_supply_demo(tmp_path):
    """examples/irrigation_supply_demo.cc builds with g++ against the C ABI and runs: without the limit VOLR goes negative; with it the
    first batch of columns, which asks for half a day's demand of a channel that holds 60 % of it, is granted in full (RATIO 1), the
    second batch half an hour later is cut back to what the first has left (RATIO < 1), and VOLR stays positive."""
    out = run_demo(build_demo("irrigation_supply_demo", tmp_path), timeout=120)
    text = out.stdout
    print(text)
    free, limited = text[text.index("without the limit"):text.index("with the limit")], text[text.index("with the limit"):]
    assert float(free.strip().splitlines()[-1].split()[-2]) < 0.0
    assert float(limited.strip().splitlines()[-1].split()[-2]) > 0.0 and "unmet demand:" in limited
    steps = [ln.split() for ln in limited.splitlines()[2:] if ln[:4].strip().isdigit()]
    day1 = steps[:12]
    assert [s[1] for s in day1[:3]] == ["5:30", "6:00", "6:30"]
    assert float(day1[1][5]) == 1.0 and 0.0 < float(day1[2][5]) < 1.0
    assert 0.0 < float(day1[2][3]) < float(day1[2][2])  # the second batch was promised what the first left
    day2 = steps[12:]
    assert 0.0 < float(day2[1][5]) < 1.0 and float(day2[1][2]) < float(day1[1][2])  # the next morning the channel is nearly empty
