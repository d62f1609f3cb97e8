"""Irrigation on the device (include/elmk.h "irrigation"): k_irrigation against the host restatement (irrigation.step) bit for bit in
both builds, after elmk_timestep7 and after elmk_timestep7_fused, over fifty chained steps on generated columns that take every branch;
the split step with the stage in it against elmk_advance_physics; the stage inside elmk_run against the stepwise calls, graph on and
off, with the closed water budget taking the term; exact restarts with a QIRRIG tape; every refusal; the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.hydrology_cases import _new, clear_snow, prepare
from tests.irrigation_cases import CHAIN_STEPS, chain_tod, generated, smpso_of
from tests.parity_cases import WETLAND
from tests.run_cases import DT, NREC, SERIES, _inputs, assert_same, device, same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

WB_FIELDS = hy.WB_READS + ("dtbegin_column_h2o",)


def _enable(D, sched):
    before = D.device_bytes
    D.irrigation_enable(sched)
    assert D.device_bytes - before == (3 * 8 + 4) * D.level_stride
    return D


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["timestep7", "fused"])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, 193, 600])
def test_fifty_chained_steps_equal_the_restatement(n, lib_path, fused):
    """The seven wrappers, then the stage, fifty times (a day and two steps of 1800 s): after every stage the three rows and the two
    state fields against irrigation.step on what the device held before it; the fields the stage reads are only read, and at five of
    the steps every other field is untouched as well.  At 600 columns the census shows every branch of A and B taken
    (tests/test_irrigation_host.py shows the same on the CPU); one column is an irrigated one that checks and applies."""
    cols, scal, soil, sched = generated(n, 900)
    lat, lon = synth.global_grid(n, seed=9)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    _enable(D, sched)
    assert n == 1 or D.level_stride != n
    smpso = smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    hit = {}
    rows = D.irrigation_rows()
    assert not rows.any()
    for s in range(CHAIN_STEPS):
        (st.timestep7_fused if fused else st.timestep7)(D, DT)
        fields = {k: D[k] for k in ir.READS}
        want, want_rows = ir.step(fields, rows, sched, DT, chain_tod(s), smpso, stored=stored, hit=hit)
        everything = s % 12 == 5
        others = {k: D[k] for k in D.fields if k not in ir.WRITES} if everything else {k: v for k, v in fields.items() if k not in ir.WRITES}
        D.irrigation(DT, chain_tod(s))
        rows = D.irrigation_rows()
        for w in range(ir.NROWS):
            assert bits(rows[w]) == bits(want_rows[w]), (s, "row", w)
        for k in ir.WRITES:
            assert same(D[k], want[k]), (s, k)
        for k, v in others.items():
            assert same(D[k], v), (s, k)
    part = D.irrigation_read(ir.RATE, col0=n // 2, n=n - n // 2)
    assert bits(part) == bits(rows[ir.RATE][n // 2:])
    print(f"n={n} census: {hit}")
    assert hit.get("check", 0) > 0 and hit.get("apply_uncapped", 0) + hit.get("apply_capped", 0) + hit.get("apply_zero", 0) > 0
    if n == 600:
        assert all(hit.get(b, 0) > 0 for b in ir.BRANCHES), {b for b in ir.BRANCHES if not hit.get(b)}
    D.close()


def test_the_stage_replays_from_a_captured_graph():
    """elmk_irrigation captured once on a caller's stream and replayed: every replay is one step (the rows live on the device)."""
    n = 193
    cols, scal, soil, _ = generated(n, 900)
    D = device((cols, scal, soil, *synth.global_grid(n, seed=9)))
    _enable(D, np.full(n, -1, np.int32))  # (no column checks: the replays only apply)
    st.timestep7_fused(D, DT)
    rate = np.full(n, 2.0e-4)
    D.irrigation_init(rate, np.full(n, 5.0))
    D.sync()
    with captured(D) as cap:
        D.irrigation(DT, 12 * 3600)
        cap.end()
        assert (D.irrigation_read(ir.NLEFT) == 5.0).all()  # captured, not run
        cap.replay(3)
        assert (D.irrigation_read(ir.NLEFT) == 2.0).all() and bits(D.irrigation_read(ir.QFLX_IRRIG)) == bits(rate)
    D.close()


# ---- 2. nothing irrigated: the split step is elmk_advance_physics -------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_the_split_step_without_irrigated_columns_is_advance_physics(lib_path):
    n = 600
    cols, scal, soil, _ = generated(n, 901)
    lat, lon = synth.global_grid(n, seed=9)
    A, B = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path), H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    _enable(B, np.full(n, -1, np.int32))
    B.irrigation_init(np.full(n, 1.0e-3), None)  # a rate without a window is never applied
    for s in range(3):
        for D in (A, B):
            st.kokkos_init_timestep(D)
        st.advance_physics(A, DT)
        st.timestep7_fused(B, DT)
        B.irrigation(DT, chain_tod(s))
        st.kokkos_soil_temperature(B, DT)
        st.kokkos_snow_hydrology(B, DT)
        st.kokkos_surface_fluxes(B, DT)
        for k in A.fields:
            assert same(A[k], B[k]), (s, k)
        q = B.irrigation_read(ir.QFLX_IRRIG)
        assert not q.any() and not np.signbit(q).any()
    A.close()
    B.close()


# ---- 3. the run ---------------------------------------------------------------------------------------------------------------------
NCOL = 193
NSTEPS = 8
FLAGS = st.RUN_IRRIGATION | st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE
TOL = 1.0e-9


@pytest.fixture(scope="module")
def base():
    b = _inputs(NCOL, 531)
    cols = b[0]
    clear_snow(cols)
    rows = prepare(cols, 532)
    c = np.arange(NCOL)
    cols["t_soisno"][:, 5:] = np.maximum(cols["t_soisno"][:, 5:], 276.0)
    # schedule() starts at 21:00 UTC: column c passes 06:00 local in step c % 6 of the run, or (one in seven) is not irrigated
    sched = ((32400 - 1800 * (c % 6) + 100 * (c % 5)) % 86400).astype(np.int32)
    sched[c % 7 == 3] = -1
    return b, rows, sched


def _context(base, graph, lib_path=None, irrig=True, wb=True, tape=False):
    b, rows, sched = base
    D = _new(b[0], b[1], b[2], rows, lib_path, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    if wb:
        D.water_balance_enable(TOL)
    if irrig:
        _enable(D, sched)
    if tape:
        D._tape = D.history_add_row(0, "irrigation", ir.QFLX_IRRIG, "avg")
    return D


def _snapshot(D, irrig=True):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out["hyd"], out["wb"] = D.soil_hydrology_rows(), D.water_balance_rows()
    if irrig:
        out["irr"] = D.irrigation_rows()
    return out


@pytest.fixture(scope="module")
def stepwise_result(base):
    A = _context(base, False)
    r = stepwise(A, base[0][5], schedule(NSTEPS), FLAGS)
    out = (tuple(r), r.bal, r.qirr, _snapshot(A))
    A.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(base, stepwise_result, graph):
    """Eight steps from 21:00 UTC over columns whose local clock passes 06:00 in steps 0 .. 5: elmk_run with the three flags against
    the stepwise calls in every field, row and ring row.  The ERRH2O row is hydrology.water_balance_end with the term, bit for bit;
    without the term the same budget would report q * dt."""
    want_diag, want_bal, qirr, want = stepwise_result
    steps = schedule(NSTEPS)
    assert [ir.time_of_day(float(p["decday"]), int(p["doy"])) for p in steps[:4]] == [75600, 77400, 79200, 81000]
    B = _context(base, graph)
    B.run(DT, steps, FLAGS)
    for g, w in zip(B.run_diagnostics(), want_diag):
        assert same(g, w)
    mms, nbad, first = B.run_water_balance()
    for s, (wm, wn, wf) in enumerate(want_bal):
        assert bits(mms[s]) == bits(wm) and (int(nbad[s]), int(first[s])) == (wn, wf), s
    got = _snapshot(B)
    assert_same(got, want)
    q = got["irr"][ir.QFLX_IRRIG]
    assert (q > 0.0).sum() > NCOL // 10 and (got["irr"][ir.NLEFT] > 0.0).any() and (np.array(qirr) > 0.0).any(axis=1).sum() >= NSTEPS - 1
    f = {k: B[k] for k in WB_FIELDS}
    with_term = hy.water_balance_end(f, got["hyd"], got["wb"], DT, qflx_irrig=q)
    assert bits(with_term[hy.WB_ERRH2O]) == bits(got["wb"][hy.WB_ERRH2O])
    without = hy.water_balance_end(f, got["hyd"], got["wb"], DT)
    wet = q > 0.0
    diff = (without[hy.WB_ERRH2O] - with_term[hy.WB_ERRH2O])[wet]
    assert np.abs(diff - q[wet] * DT).max() <= 16 * 2.0 ** -53 * np.abs(with_term[hy.WB_ENDWB]).max()
    assert bits(without[hy.WB_ERRH2O][~wet]) == bits(with_term[hy.WB_ERRH2O][~wet])
    B.close()


def test_an_unflagged_run_never_irrigates(base):
    """With the feature enabled but without the flag the run is the run of a context that never enabled it, and the rows stay put;
    a flagged run after it takes the stage in again (the captured step follows the flag)."""
    steps = schedule(4)
    A, B = _context(base, True, irrig=False), _context(base, True)
    B.irrigation_init(np.full(NCOL, 1.0e-3), np.full(NCOL, 4.0))
    rows0 = B.irrigation_rows()
    for D in (A, B):
        D.run(DT, steps, FLAGS & ~st.RUN_IRRIGATION)
    assert bits(B.irrigation_rows()) == bits(rows0)
    # (B's budget takes the term of the untouched QFLX_IRRIG row, +0.0: the same bits)
    assert_same(_snapshot(A, irrig=False), _snapshot(B, irrig=False))
    B.run(DT, steps[:1], FLAGS)
    assert (B.irrigation_read(ir.NLEFT) <= 3.0).any() and (B.irrigation_read(ir.QFLX_IRRIG) > 0.0).any()
    A.close()
    B.close()


# ---- 4. restart ---------------------------------------------------------------------------------------------------------------------
def test_restart_4_plus_4_equals_8(base):
    """Four steps, an image taken while windows are open (NLEFT > 0), a fresh context, four more steps: the bits of eight steps in one
    context in the state, the rows and a QIRRIG tape; the same through restart.slice and restart.merge.  The image is version 5 exactly
    when the feature is enabled; a context without it saves the version-4 image it saved before."""
    S8 = schedule(NSTEPS)
    flags = FLAGS | st.RUN_HISTORY
    A = _context(base, True, tape=True)
    A.run(DT, S8, flags)
    want, want_tape = _snapshot(A), A.history_read(A._tape)
    assert (want_tape > 0.0).any()
    A.close()
    B = _context(base, True, tape=True)
    B.run(DT, S8[:4], flags)
    assert (B.irrigation_read(ir.NLEFT) > 0.0).any()
    img = B.restart_save()
    p = R.verify(img)
    assert int(p["header"]["version"]) == R.VERSION_IRRIGATION
    irr_sections = [(int(s["id"]), int(s["nlev"])) for s in p["sections"] if int(s["kind"]) == R.IRRIGATION_SECTION]
    assert irr_sections == [(ir.RATE, 1), (ir.NLEFT, 1)]
    assert R.entry_row(p["entries"]["field"][0]) == (st.ROWS_IRRIGATION, ir.QFLX_IRRIG)
    size_with = B.restart_size()
    B.close()
    # without the feature: version 4, and smaller by the two sections (and what the table entries add to the header, if anything)
    P = _context(base, True, irrig=False)
    P.history_add_row(0, "hydrology", hy.ZWT, "avg")  # (the same number of entries)
    size_without = P.restart_size()
    assert int(R.verify(P.restart_save())["header"]["version"]) == R.VERSION_HYDROLOGY
    sec = (NCOL * 8 + 255) // 256 * 256
    assert 2 * sec <= size_with - size_without <= 2 * sec + 256
    before = {k: P[k] for k in P.fields}
    with pytest.raises(L.ElmkError, match="irrigation"):
        P.restart_load(img)
    assert all(same(P[k], v) for k, v in before.items())
    # enabled and cleared again: the size it had
    P.history_clear()
    size_plain = P.restart_size()
    _enable(P, base[2])
    assert P.restart_size() > size_plain
    P.irrigation_clear()
    assert P.restart_size() == size_plain
    P.close()
    halves = [R.slice(img, 0, 100), R.slice(img, 100, NCOL - 100)]
    merged = R.merge(halves[::-1])
    assert bits(merged) == bits(img)
    for image in (img, merged):
        Cx = _context(base, True, tape=True)
        Cx.restart_load(image)
        Cx.run(DT, S8[4:], flags)
        assert_same(_snapshot(Cx), want)
        assert bits(Cx.history_read(Cx._tape)) == bits(want_tape)
        Cx.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(base):
    """Every refusal of the feature: afterwards elmk_device_bytes, the image size, every field and every row are what they were, and a
    following step gives the bits of a context that met no refusal.  A history row entry bars the clear."""
    b, rows, sched = base
    S1 = schedule(1)
    nan, inf = float("nan"), float("inf")

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    D, W = _context(base, True, irrig=False), _context(base, True)
    bytes0, size0 = D.device_bytes, D.restart_size()
    before = _snapshot(D, irrig=False)
    bad_sched = [np.where(np.arange(NCOL) == 7, v, sched).astype(np.int32) for v in (-2, 86400, 2 ** 31 - 1)]
    refused(lambda: D.irrigation(DT, 0), lambda: D.irrigation_init(), lambda: D.irrigation_read(0), match="not enabled")
    refused(lambda: D.run(DT, S1, FLAGS), lambda: D.history_add_row(0, "irrigation", ir.QFLX_IRRIG, "avg"),
            *(lambda s=s: D.irrigation_enable(s) for s in bad_sched))
    D.irrigation_clear()  # nothing to free: OK
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(_snapshot(D, irrig=False), before)
    # a stream being captured
    with captured(D) as cap:
        s32 = np.ascontiguousarray(sched, dtype=np.int32)
        rc = D.lib.elmk_irrigation_enable(D.ctx, s32.ctypes.data_as(C.c_void_p))
        cap.end()
        assert rc == -1 and D.device_bytes == bytes0

    _enable(D, sched)
    bytes1, size1 = D.device_bytes, D.restart_size()
    D.irrigation_init(np.full(NCOL, 1.0e-4), np.full(NCOL, 2.0))
    W.irrigation_init(np.full(NCOL, 1.0e-4), np.full(NCOL, 2.0))
    state1 = _snapshot(D)
    col = lambda v, fill: np.where(np.arange(NCOL) == NCOL - 1, v, fill)  # noqa: E731
    refused(lambda: D.irrigation_enable(sched), match="already enabled")
    refused(*(lambda dt=dt: D.irrigation(dt, 0) for dt in (0.0, -1800.0, 1800.5, nan, inf, 86401.0)),
            *(lambda t=t: D.irrigation(DT, t) for t in (-1, 86400)),
            *(lambda v=v: D.irrigation_init(None, col(v, 1.0)) for v in (0.5, -1.0, 86401.0, nan, inf)),
            *(lambda v=v: D.irrigation_init(col(v, 1.0e-4), None) for v in (nan, inf, -inf, -1.0e-9)),
            lambda: D.irrigation_read(3), lambda: D.irrigation_read(-1), lambda: D.irrigation_read(0, col0=NCOL, n=1),
            lambda: D.irrigation_read(0, col0=NCOL - 1, n=2), lambda: D.irrigation_read(0, col0=-1, n=1),
            lambda: D.run(DT + 0.5, S1, FLAGS), lambda: D.history_add_row(0, "irrigation", 3, "avg"))
    assert D.device_bytes == bytes1 and D.restart_size() == size1
    assert_same(_snapshot(D), state1)
    # a row entry of the family bars the clear
    D.history_add_row(0, "irrigation", ir.QFLX_IRRIG, "avg")
    size_e, bytes_e = D.restart_size(), D.device_bytes
    refused(D.irrigation_clear, match="elmk_history_clear first")
    assert D.device_bytes == bytes_e and D.restart_size() == size_e
    assert_same(_snapshot(D), state1)
    D.history_clear()
    assert D.restart_size() == size1
    # a land unit that is not soil or crop: nothing is enqueued
    D.set_land(**WETLAND)
    D.irrigation(DT, 0)
    assert_same(_snapshot(D), state1)
    D.set_land(**synth.TEST_LAND)
    # the following step
    for X in (D, W):
        X.run(DT, S1, FLAGS)
    assert_same(_snapshot(D), _snapshot(W))
    assert (D.irrigation_read(ir.QFLX_IRRIG) == 1.0e-4).all()
    D.irrigation_clear()
    refused(lambda: D.irrigation_read(0), match="not enabled")
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    D.close()
    W.close()


# ---- 6. the demo --------------------------------------------------------------------------------------------------------------------
def test_irrigation_demo(tmp_path):
    """examples/irrigation_demo.cc builds with g++ against the C ABI and runs: on the first morning the check sets a rate and NLEFT counts
    down from 8 while QIRRIG is applied; on the second morning the column is unstressed."""
    out = run_demo(build_demo("irrigation_demo", tmp_path), timeout=120)
    lines = out.stdout.strip().splitlines()
    assert "irrigation, 96 steps" in lines[0] and lines[-1].startswith("applied to column 0:")
    steps = [ln.split() for ln in lines[2:-1]]
    assert len(steps) == 2 * 12
    day1 = steps[:12]
    assert [s[1] for s in day1[:3]] == ["5:00", "5:30", "6:00"]
    nleft = [int(s[4]) for s in day1]
    assert nleft == [0, 0, 8, 7, 6, 5, 4, 3, 2, 1, 0, 0]
    rate = float(day1[2][3])
    assert rate > 0.0 and [float(s[5]) for s in day1] == [0.0, 0.0, 0.0] + [rate] * 8 + [0.0]
    assert float(day1[0][2]) < 0.5 and float(day1[-1][2]) > float(day1[0][2])
    day2 = steps[12:]
    assert all(int(s[4]) == 0 and float(s[5]) == 0.0 and float(s[2]) >= 0.999999 for s in day2)  # wet enough: no check, nothing applied
    assert abs(float(lines[-1].split()[-2]) - rate * 1800.0 * 8) < 1.0e-2
