"""Multi-step runs on the device (elmk_run, include/elmk.h "multi-step runs"): every run is compared bit for bit with the same steps
driven through the existing calls ("stepwise": the atm_* and mlai .. mhbot fields uploaded from the same host records before every
step, elmk_solar_geometry, elmk_phenology, elmk_get_forcing, elmk_init_timestep, elmk_advance_physics, then
elmk_evaluate_conservation and elmk_error_summary after every step)."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from tests import helpers as H
from tests.hydrology_cases import clear_snow, prepare
from tests.run_cases import (DT, NREC, NSTEPS, SERIES, _inputs, _pair, assert_same_rows, assert_same_state, demo_records, schedule,
                             stepwise, upload_series)
from tests.support import build_demo, captured, run_demo, same, state_blob

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base():
    return _inputs(5003, 71)


def test_run_equals_stepwise_graph_on(base):
    """Twelve steps as one elmk_run replayed from one captured step: state, err_flags, conservation and flag rows bit for bit."""
    cols, _, _, _, _, rec = base
    A, B = _pair(base)
    steps = schedule()
    want = stepwise(A, rec, steps)
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    B.run(DT, steps)
    got = B.run_diagnostics()
    assert_same_rows(got, want)
    assert_same_state(A, B, cols)
    assert len(np.unique(want[0][:, 6, 2])) > 1  # the steps differ
    A.close()
    B.close()


def test_graph_off_equals_graph_on(base):
    cols, _, _, _, _, rec = base
    A, B = _pair(base, graph=False)
    B.set_graph(True)
    steps = schedule()
    for D in (A, B):
        D.run_reserve(NREC, NSTEPS)
        upload_series(D, rec)
        D.run(DT, steps)
    assert_same_rows(A.run_diagnostics(), B.run_diagnostics())
    for name in A.fields:
        assert same(A[name], B[name]), name
    A.close()
    B.close()


def test_two_runs_with_an_upload_between_equal_one_run(base):
    """Runs of 5 + 7 steps enqueued back to back: between them the second window is uploaded, and slot 3 - which the first run
    reads - is replaced by new values.  The upload must wait for the first run, so that the first run sees the old record and the
    second the new one, as the stepwise reference does.  (An upload that did not wait would most likely land before the first run's
    last steps read slot 3 and change their bits; the check relies on that timing, it cannot force it.)"""
    cols, _, _, _, _, rec = base
    A, B = _pair(base)
    steps = schedule()
    late = {k: v.copy() for k, v in rec.items()}
    for k in st.SERIES_FORCING:
        late[k][3] = rec[k][3] * 1.001 + (30.0 if k == "atm_flds" else 0.0)
    want = stepwise(A, rec, steps, rec_late=late, late_from=5)
    B.run_reserve(NREC, 8)
    upload_series(B, rec, forc_slots=range(0, 4))  # steps 0..4 read slots 0..3
    B.run(DT, steps[:5])
    for k in st.SERIES_FORCING:
        B.series_upload(k, 3, late[k][3:NREC])  # slot 3 (read by the run in flight) and the second window
    B.run(DT, steps[5:])
    got = B.run_diagnostics()
    assert_same_rows(got, tuple(w[5:] for w in want))
    assert_same_state(A, B, cols)
    A.close()
    B.close()


def test_third_run_keeps_the_first_runs_records(base):
    """Three runs of 4 steps enqueued back to back without a sync (the third reuses the first one's step table), then slots 0 and
    1 - read by the first run only - are replaced by other values: the upload may not write under the first run, so all twelve
    steps give the stepwise bits of the original records."""
    cols, _, _, _, _, rec = base
    A, B = _pair(base)
    steps = schedule()
    want = stepwise(A, rec, steps)
    B.run_reserve(NREC, 4)
    upload_series(B, rec)
    for r in range(3):
        B.run(DT, steps[4 * r:4 * r + 4])  # slots read: 0..2, 2..4, 4..6
    for k in st.SERIES_FORCING:
        B.series_upload(k, 0, rec[k][0:2] * 0.5 + (40.0 if k == "atm_flds" else 0.0))
    got = B.run_diagnostics()
    assert_same_rows(got, tuple(w[8:] for w in want))
    assert_same_state(A, B, cols)
    A.close()
    B.close()


ENTRIES = [(0, "t_grnd", "avg"), (0, "eflx_sh_tot", "sum"), (1, "t_grnd", "max"), (1, "h2osoi_liq", "min"), (2, "snl", "inst"),
           (2, "t_soisno", "avg")]


def test_history_option_equals_stepwise_accumulate(base):
    cols, _, _, _, _, rec = base
    A, B = _pair(base)
    ids = [[D.history_add(t, f, op) for t, f, op in ENTRIES] for D in (A, B)]
    steps = schedule()
    stepwise(A, rec, steps, st.RUN_HISTORY)
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    B.run(DT, steps, st.RUN_HISTORY)
    for a, b in zip(*ids):
        assert same(A.history_read(a), B.history_read(b))
    for t in range(3):
        assert A.history_count(t) == B.history_count(t) == NSTEPS
    assert_same_state(A, B, cols)
    A.close()
    B.close()


def test_qbot_is_rh_option_equals_stepwise(base):
    cols, _, _, _, _, rec = base
    rec = dict(rec)
    rec["atm_qbot"] = np.clip(rec["atm_qbot"] * 5000.0, 5.0, 100.0)  # relative humidity, percent
    A, B = _pair(base)
    steps = schedule()
    want = stepwise(A, rec, steps, st.RUN_QBOT_IS_RH)
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    B.run(DT, steps, st.RUN_QBOT_IS_RH)
    assert_same_rows(B.run_diagnostics(), want)
    assert_same_state(A, B, cols)
    A.close()
    B.close()


def test_refusals_enqueue_nothing(base):
    """Every refusal of elmk_run returns ELMK_E_INVALID, and after each one a valid run from the same starting state (restored
    from a snapshot of every field) still gives the bits of the stepwise run."""
    cols, _, _, _, _, rec = base
    A, B = _pair(base)
    steps = schedule()
    want = stepwise(A, rec, steps)
    want_state = {name: A[name] for name in A.fields if name not in SERIES}
    B.snapshot_fields(list(B.fields))

    def refused(dt, s, flags=0):
        a = np.ascontiguousarray(s, dtype=st.RUN_STEP_DTYPE)
        return B.lib.elmk_run(B.ctx, float(dt), a.ctypes.data_as(C.c_void_p), int(a.size), int(flags)) == -1

    def valid_run_still_gives_the_bits(what):
        B.restore_fields()
        B.run(DT, steps)
        assert_same_rows(B.run_diagnostics(), want)
        for name, v in want_state.items():
            assert same(B[name], v), (what, name)
        for name in SERIES:
            assert same(B[name], np.ascontiguousarray(cols[name], dtype=B[name].dtype)), (what, name)

    assert refused(DT, steps)  # not reserved
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    assert B.run_diagnostics()[0].shape == (0, 8, 3)  # no run was ever enqueued
    valid_run_still_gives_the_bits("not reserved")
    cases = [("nsteps 0", DT, steps[:0], 0), ("nsteps > max_steps", DT, np.concatenate([steps, steps[:1]]), 0)]
    cases += [(f"dt {dt}", dt, steps, 0) for dt in (0.0, -DT, float("nan"), float("inf"))]
    for slot in (-1, NREC - 1):
        s = steps.copy()
        s[4]["forc_slot"] = slot
        cases.append((f"forc_slot {slot}", DT, s, 0))
    for f in ("month1", "month2"):
        for m in (-1, 12):
            s = steps.copy()
            s[7][f] = m
            cases.append((f"{f} {m}", DT, s, 0))
    cases.append(("flags 4", DT, steps, 4))
    for what, dt, s, flags in cases:
        assert refused(dt, s, flags), what
        valid_run_still_gives_the_bits(what)
    with captured(B):
        rc = refused(DT, steps)
    assert rc
    valid_run_still_gives_the_bits("stream being captured")
    A.close()
    B.close()


def test_the_captured_step_follows_every_part_of_its_key():
    """One context replays its run step from a captured graph, the other enqueues it stage by stage.  Between two-step runs one part of
    what the step depends on changes at a time: each run flag, the history and the accumulator tables (an entry more under the same
    flags), the shortwave mode, the downscaling mode without and with groups, and back.  After every run every field, the diagnostics
    rows, every history and accumulator read and the rows of the active layer and the soil hydrology are bit-equal: a graph kept past
    a change of its key would hold the stages, kernels or tables of the moment it was captured.  (The land unit under
    ELMK_RUN_HYDROLOGY: test_gpu_hydrology.test_the_captured_run_step_follows_the_land_unit.  The three newer flags and the rest of
    the key, with every stage on: test_gpu_full_step.py.)"""
    from elmkernels_amd import hydrology as hy
    from elmkernels_amd import regrid as RG

    n = 200  # the base fixture is larger; two blocks of most kernels with a ragged tail
    inputs = _inputs(n, 75)
    clear_snow(inputs[0])
    rows = prepare(inputs[0], 76)
    cols, scal, soil, lat, lon, rec = inputs
    pair = [H.device_state(cols, scal, soil, lat=lat, lon=lon) for _ in range(2)]
    for D, graph in zip(pair, (True, False)):
        D.set_graph(graph)
        D.run_reserve(NREC, 2)
        upload_series(D, rec)
    rng = np.random.default_rng(77)
    hf = 200.0 + 1500.0 * rng.random(n)
    hc = hf + rng.uniform(-1500.0, 1500.0, n)
    cell = np.arange(n) // 60
    cell[n - 9:] = -1  # columns in no group
    groups = RG.owner_map(cell, 0.5 + rng.random(n), int(cell.max()) + 1)
    deposition = 1.0e-12 * (1.0 + rng.random((12, n)))
    hist, accum = {}, set()  # the entry ids (history: with the tape), the same in both contexts

    def add_history(D, tape, field, op):
        hist[D.history_add(tape, field, op)] = tape

    def add_accum(D, *entry):
        accum.add(D.accum_add(*entry))

    def aerosol(D):
        D.aerosol_reserve()
        D.aerosol_upload("bcphi", 0, deposition)

    def active_layer(D):
        D.active_layer_enable()
        D.active_layer_init()

    def hydrology(D):
        D.soil_hydrology_enable()
        D.soil_hydrology_set_params(rows[hy.HKSAT:hy.HKSAT + hy.N], rows[hy.WTFACT], rows[hy.H2OSFC_THRESH], rows[hy.K_WET], rows[hy.RSUB_TOP_MAX])
        D.soil_hydrology_init(rows[hy.ZWT], rows[hy.WA])

    def coszen(D):
        D.set_shortwave_mode("coszen", 3600.0)
        D.series_record_times(0, 14.875 + np.arange(NREC) / 24.0)

    def topo(D):
        D.set_column_elevation(hc, hf)
        D.set_downscaling("topo")

    F = st
    steps = [  # (what changes, the flags from here on, the change)
        ("nothing: the first capture", 0, None),
        ("QBOT_IS_RH", F.RUN_QBOT_IS_RH, None),
        ("flags back to 0", 0, None),
        ("HISTORY with one entry", F.RUN_HISTORY, lambda D: add_history(D, 0, "t_grnd", "avg")),
        ("a history entry more", F.RUN_HISTORY, lambda D: add_history(D, 1, "t_soisno", "max")),  # (tape 0 holds samples)
        ("ACCUM with one entry", F.RUN_HISTORY | F.RUN_ACCUM, lambda D: add_accum(D, "t_grnd", "runmean", 3)),
        ("an accumulator entry more", F.RUN_HISTORY | F.RUN_ACCUM, lambda D: add_accum(D, "h2osoi_liq", "timeavg", 2)),
        ("AEROSOL", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_AEROSOL, aerosol),
        ("ALT", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_AEROSOL | F.RUN_ALT, active_layer),
        ("ALT flag off, the rows stay", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_AEROSOL, None),
        ("HYDROLOGY", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT | F.RUN_HYDROLOGY, hydrology),
        ("HYDROLOGY flag off", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, None),
        ("shortwave COSZEN", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, coszen),
        ("downscaling TOPO", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, topo),
        ("downscaling groups", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, lambda D: D.set_downscaling_groups(*groups)),
        ("groups cleared", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, lambda D: D.clear_downscaling_groups()),
        ("downscaling off", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, lambda D: D.set_downscaling("off")),
        ("shortwave REFERENCE", F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_ALT, lambda D: D.set_shortwave_mode("reference")),
        ("the six older flags", F.RUN_QBOT_IS_RH | F.RUN_HISTORY | F.RUN_ACCUM | F.RUN_AEROSOL | F.RUN_ALT | F.RUN_HYDROLOGY, None),
        ("flags back to 0 again", 0, None),
    ]
    sch = schedule()
    for k, (what, flags, change) in enumerate(steps):
        for D in pair:
            if change:
                change(D)
            D.run(DT, sch[2 * (k % 6):2 * (k % 6) + 2], flags)
        A, B = pair
        assert_same_rows(A.run_diagnostics(), B.run_diagnostics())
        for name in A.fields:
            assert same(A[name], B[name]), (what, name)
        for e, tape in sorted(hist.items()):
            assert A.history_count(tape) == B.history_count(tape) > 0
            assert same(A.history_read(e), B.history_read(e)), (what, "history", e)
        for e in sorted(accum):
            (va, na), (vb, nb) = A.accum_read(e), B.accum_read(e)
            assert na == nb and same(va, vb), (what, "accumulator", e)
        if flags & F.RUN_ALT or "ALT" in what:
            assert all(same(A.active_layer_read(w), B.active_layer_read(w)) for w in range(3)), what
        if flags & F.RUN_HYDROLOGY or "HYDROLOGY" in what:
            assert same(A.soil_hydrology_rows(), B.soil_hydrology_rows()), what
    for D in pair:
        D.close()


@pytest.mark.parametrize("half", [False, True])
def test_large_launch_run_equals_stepwise(half):
    """262 144 columns (the benchmark's launch structure), three steps; ELMK_OPT_CF_HALF_WORKGROUPS off and on."""
    cols, scal, soil, lat, lon, rec = _inputs(262144, 72)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    for D in (A, B):
        D.set_graph(True)
        D.set_option(st.OPT_CF_HALF_WORKGROUPS, int(half))
    steps = schedule(3)
    want = stepwise(A, rec, steps)
    B.run_reserve(NREC, 3)
    upload_series(B, rec)
    B.run(DT, steps)
    assert_same_rows(B.run_diagnostics(), want)
    assert_same_state(A, B, cols)
    A.close()
    B.close()


def test_fp32_state_library():
    cols, scal, soil, lat, lon, rec = _inputs(2053, 73)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=L.F32_LIB_PATH)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=L.F32_LIB_PATH)
    assert B.lib.elmk_state_real_bytes() == 4
    steps = schedule()
    want = stepwise(A, rec, steps)
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    B.run(DT, steps)
    assert_same_rows(B.run_diagnostics(), want)
    for name in A.fields:
        if name in SERIES:
            assert same(B[name], np.ascontiguousarray(cols[name], dtype=B[name].dtype).astype(np.float32).astype(B[name].dtype)), name
        else:
            assert same(A[name], B[name]), name
    A.close()
    B.close()


def test_run_demo(tmp_path):
    """examples/run_demo.cc (48 half-hour steps over 25 hourly records as two runs of 24, the second window uploaded during the
    first run) writes the PrimaryVars and the 48 conservation rows of the stepwise run, bit for bit."""
    n, nsteps = 3008, 48
    cols, scal, soil, lat, lon, rec = _inputs(n, 74, nrec=25)
    steps = schedule(nsteps)
    exe = build_demo("run_demo", tmp_path)
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, demo_records(lat, lon, rec) + [("steps", steps)]))
    r = run_demo(exe, tmp_path / "state.bin", tmp_path / "out.bin")
    assert "48 steps" in r.stdout, r.stdout
    # the same steps through the Python layer, stepwise
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_graph(True)
    cons, _, _ = stepwise(D, rec, steps)
    raw = (tmp_path / "out.bin").read_bytes()
    off = 0
    for name in st.ELMInterface.PRIMARY_VARS:
        want = D[name]
        got = np.frombuffer(raw, want.dtype, want.size, off).reshape(want.shape)
        off += want.nbytes
        assert same(got, want), name
    got = np.frombuffer(raw, np.float64, nsteps * 24, off).reshape(nsteps, 8, 3)
    assert same(got, cons)
    assert off + nsteps * 24 * 8 == len(raw)
    D.close()
