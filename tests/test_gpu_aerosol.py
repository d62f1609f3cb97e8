"""Aerosol deposition on the device (include/elmk.h "aerosol deposition"): k_aerosol_deposition against aerosol.interpolate bit for bit
in both builds, elmk_run with ELMK_RUN_AEROSOL against the stepwise calls, a second device path, the flag beside the others,
restarts, every refusal, and the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import accum
from elmkernels_amd import aerosol
from elmkernels_amd import regrid
from elmkernels_amd import state as st
from tests import helpers as H
from tests.run_cases import DT, NREC, NSTEPS, SERIES, _inputs, demo_records, schedule, stepwise, upload_series
from tests.support import build_demo, captured, run_demo, same, state_blob

pytestmark = pytest.mark.gpu

N, NCELLS, SEED = 193, 7, 81
AER = aerosol.FIELDS
CALLS = [(11, 0, 0.3, 0.7), (4, 4, 0.25, 0.75), (0, 1, 1.0, 0.0), (6, 7, 0.0, 1.0)]


def make_map(kind, n, ncells=NCELLS, seed=5):
    """"col": per-column series (NPTS 0); "n1": one term per column with a weight that is not 1; "n3": three rows with -1 padding in
    rows 1 and 2 (the library pads them to four); "n2": two rows, row 1 padding in about 40 % of the columns; "n5": five rows with
    padding in rows 1 .. 4 (padded to eight); "n8": eight rows, full in most columns.  In all of them column 0 has padding in every
    row but the first and column 3 has none, and the weights are no partition of one."""
    if kind == "col":
        return n, None, None
    rng = np.random.default_rng(seed)
    if kind == "n1":
        return ncells, rng.integers(0, ncells, (1, n)).astype(np.int32), rng.random((1, n)) + 0.5
    if kind in ("n2", "n5", "n8"):
        npts = int(kind[1:])
        idx = rng.integers(0, ncells, (npts, n)).astype(np.int32)
        w = rng.random((npts, n)) + 0.1
        for k in range(1, npts):
            idx[k, rng.random(n) < (0.1 if kind == "n8" else 0.4)] = -1
        idx[1:, 0] = -1
        if n > 3:
            idx[1:, 3] = (2 + 3 * np.arange(npts - 1)) % ncells
        return ncells, idx, w
    idx = rng.integers(0, ncells, (3, n)).astype(np.int32)
    w = rng.random((3, n)) + 0.1
    idx[1, rng.random(n) < 0.4] = -1
    idx[2, rng.random(n) < 0.5] = -1
    idx[1:, 0] = -1
    if n > 3:
        idx[1, 3], idx[2, 3] = 2, 5
    return ncells, idx, w


def expected_bytes(D, ncells, idx):
    """The formula of include/elmk.h: the series, and with a map its idx and w rows, each rounded up to 256 bytes."""
    up = lambda b: (b + 255) // 256 * 256  # noqa: E731
    total = up(11 * 12 * ncells * 8)
    if idx is not None:
        npts = idx.shape[0]
        npad = 1 if npts <= 1 else 2 if npts <= 2 else 4 if npts <= 4 else 8
        total += up(npad * 4 * D.level_stride) + up(npad * 8 * D.level_stride)
    return total


def reserve_and_upload(D, ncells, idx, w, series, months=range(12)):
    D.aerosol_reserve(ncells, idx, w)
    months = list(months)
    for s in aerosol.STREAMS:
        for m in months:
            D.aerosol_upload("aer_" + s, m, series[s][m])


def stored(D, a):
    """The fp64 value as the build stores and returns it."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if D.lib.elmk_state_real_bytes() == 4 else a


# ---- 1. the kernel equals the restatement ---------------------------------------------------------------------------------------------
KINDS = ("col", "n1", "n2", "n3", "n5", "n8")  # NPTS 0, 1, 2, 4, 8, 8
# one thread per column, 256 per workgroup: one column, 193, a workgroup and one column in every width and both builds; the widths at
# the ends, 0 and 8, also at one whole workgroup (the level stride unpadded) and at three with a partial last wave
KERNEL_CASES = ([(n, k, p) for p in (None, L.F32_LIB_PATH) for k in KINDS for n in (1, N, 257)] +
                [(n, k, None) for k in ("col", "n8") for n in (256, 600)])


@pytest.mark.parametrize("n,kind,lib_path", KERNEL_CASES, ids=[f"{n}-{k}-{'fp32state' if p else 'fp64'}" for n, k, p in KERNEL_CASES])
def test_kernel_equals_the_restatement(n, kind, lib_path):
    """The stepwise call against aerosol.interpolate after every deposition, and what it must not touch: every other field.  (No read
    that the wrapper offers reaches a row's padding past ncols.)"""
    cols, scal, soil, lat, lon, _ = _inputs(n, SEED)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    assert (D.level_stride == n) == (n == 256) and D.level_stride >= n
    ncells, idx, w = make_map(kind, n)
    if idx is not None and n > 3:
        assert (idx[1:, 0] == -1).all() and (idx[:, 3] >= 0).all()
    series = aerosol.synthetic_climatology(ncells, seed=3)
    for s in aerosol.STREAMS:
        series[s][8:11] = 0.0  # months 8 .. 10 are never uploaded: they read as zero
    bytes0 = D.device_bytes
    D.aerosol_reserve(ncells, idx, w)
    assert D.device_bytes - bytes0 == expected_bytes(D, ncells, idx)
    D.aerosol_deposition(2, 9, 0.5, 0.5)  # nothing uploaded yet: every stream reads zero
    for f in AER:
        assert not D[f].any(), f
    for f in AER:  # what was there before must not show through
        D.upload(f, cols[f])
    for s in aerosol.STREAMS:
        D.aerosol_upload(s, 0, series[s][0:8])
        D.aerosol_upload("aer_" + s, 11, series[s][11])
    others = {k: D[k] for k in D.fields if k not in AER}
    for m1, m2, wt1, wt2 in CALLS + [(7, 8, 0.5, 0.5), (9, 10, 1.0, 1.0)]:
        D.aerosol_deposition(m1, m2, wt1, wt2)
        want = aerosol.interpolate(series, m1, m2, wt1, wt2, idx, w)
        for s in aerosol.STREAMS:
            assert same(D["aer_" + s], stored(D, want[s])), (s, m1, m2)
    D.aerosol_deposition(0, 1, 0.4, 0.6)
    assert D["aer_dst4_2"].any()
    for k, v in others.items():
        assert same(D[k], v), k
    D.aerosol_clear()
    assert D.device_bytes == bytes0
    D.close()


# ---- 2. the run equals the stepwise calls ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return _inputs(N, SEED)


@pytest.fixture(scope="module")
def mapped():
    ncells, idx, w = make_map("n3", N)
    return ncells, idx, w, aerosol.synthetic_climatology(ncells, seed=9)


def stepwise_device(D, rec, steps, history=False, update_accum=False):
    """tests/run_cases.py: stepwise with elmk_aerosol_deposition before elmk_init_timestep, where elmk_run has it."""
    cons, fo, fb = [], [], []
    for p in steps:
        D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
        f = int(p["forc_slot"])
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([rec[k][f], rec[k][f + 1]], axis=1))
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"])
        D.aerosol_deposition(int(p["month1"]), int(p["month2"]), float(p["month_wt1"]), float(p["month_wt2"]))
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        cons.append(st.kokkos_evaluate_conservation(D, DT))
        flags, first = D.error_summary()
        fo.append(flags)
        fb.append(first)
        if update_accum:
            D.accum_update()
        if history:
            D.history_accumulate()
    return np.array(cons), np.array(fo, np.uint32), np.array(fb, np.int64)


def run_context(base, mapped, graph, lib_path=None):
    cols, scal, soil, lat, lon, rec = base
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    D.set_graph(graph)
    D.run_reserve(NREC, NSTEPS)
    upload_series(D, rec)
    if mapped is not None:
        reserve_and_upload(D, *mapped)
    return D


def state_of(D):
    return {k: D[k] for k in D.fields if k not in SERIES}


def assert_states(a, b, what=""):
    for k, v in a.items():
        assert same(v, b[k]), (what, k)


@pytest.fixture(scope="module")
def flagged(base, mapped):
    """The 12-step run with ELMK_RUN_AEROSOL, graph off: (diagnostics rows, every field but the series inputs)."""
    B = run_context(base, mapped, False)
    B.run(DT, schedule(), st.RUN_AEROSOL)
    out = B.run_diagnostics(), state_of(B)
    B.close()
    return out


def test_run_equals_stepwise(base, mapped, flagged):
    cols, scal, soil, lat, lon, rec = base
    ncells, idx, w, series = mapped
    steps = schedule()
    assert {(int(p["month1"]), int(p["month2"])) for p in steps} == {(11, 0), (0, 1)}
    snow0 = cols["snl"].reshape(-1) > 0
    assert snow0.any()  # (from synth.make_state: no GPU needed to know it)
    # A: the existing calls, the host-interpolated aer_* uploaded before every step
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    rows = []
    for p in steps:
        want = aerosol.interpolate(series, p["month1"], p["month2"], p["month_wt1"], p["month_wt2"], idx, w)
        for s in aerosol.STREAMS:
            A.upload("aer_" + s, want[s])
        rows.append(stepwise(A, rec, steps[[len(rows)]]))
    want_rows = tuple(np.concatenate([r[i] for r in rows]) for i in range(3))
    want_state = state_of(A)
    A.close()
    # A2: the same with the device's stepwise call
    A2 = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    reserve_and_upload(A2, ncells, idx, w, series)
    rows2 = stepwise_device(A2, rec, steps)
    assert_states(want_state, state_of(A2), "stepwise device call")
    A2.close()
    # B: one run, graph off; B': graph on
    got_rows, got_state = flagged
    Bg = run_context(base, mapped, True)
    Bg.run(DT, steps, st.RUN_AEROSOL)
    for got, what in ((got_rows, "graph off"), (Bg.run_diagnostics(), "graph on"), (rows2, "stepwise device call")):
        for g, wnt in zip(got, want_rows):
            assert same(g, wnt), what
    assert_states(want_state, got_state, "graph off")
    assert_states(want_state, state_of(Bg), "graph on")
    for k in SERIES:  # a run reads neither atm_* nor mlai .. mhbot
        assert same(Bg[k], np.ascontiguousarray(cols[k], dtype=Bg[k].dtype)), k
    Bg.close()
    # C: without the flag aer_* are read-only
    Cx = run_context(base, mapped, False)
    Cx.run(DT, steps)
    for f in AER:
        assert same(Cx[f], np.ascontiguousarray(cols[f], dtype=np.float64)), f
    # not vacuous: snow layers during the run, and the deposition reaches the snow aerosol mass
    snow = snow0 & (got_state["snl"].reshape(-1) > 0)
    assert snow.any()
    differs = (got_state["mss_dst1"] != Cx["mss_dst1"]).any(axis=1)
    assert (differs & snow).any()
    assert not same(got_state["aer_dst1_1"], Cx["aer_dst1_1"])
    Cx.close()


# ---- 2b. the run form at every width: k_aerosol_deposition<NPTS, true> ---------------------------------------------------------------
NW, WIDE_STEPS = 257, 4  # a workgroup and one column; four steps of the (11, 0) bracket, each with weights of its own


@pytest.fixture(scope="module")
def wide():
    return _inputs(NW, SEED)


@pytest.fixture(scope="module")
def wide_unflagged(wide):
    """The same steps without the flag (and without a series): every field but the series inputs."""
    U = run_context(wide, None, False)
    U.run(DT, schedule()[:WIDE_STEPS])
    out = state_of(U)
    U.close()
    return out


@pytest.mark.parametrize("graph", [False, True], ids=["nograph", "graph"])
@pytest.mark.parametrize("kind", ["n1", "n2", "n8"])
def test_run_deposits_the_last_steps_bracket_at_every_width(wide, wide_unflagged, kind, graph):
    """No kernel of the step writes the eleven aer_* fields (class SURFACE), so after a flagged run they hold what the run's form of
    the kernel wrote in the last step: aerosol.interpolate of that step's row of the schedule, at state precision.  test_run_equals_
    stepwise has the width 4 (and test_history_accum_and_aerosol_flags_together no other)."""
    ncells, idx, w = make_map(kind, NW)
    series = aerosol.synthetic_climatology(ncells, seed=13)
    steps = schedule()[:WIDE_STEPS]
    last = steps[-1]
    assert (int(last["month1"]), int(last["month2"])) == (11, 0) and 0.0 < float(last["month_wt1"]) < float(last["month_wt2"]) < 1.0
    assert len({float(p["month_wt1"]) for p in steps}) == WIDE_STEPS  # (an earlier step's row would give other numbers)
    assert all(st.field_class(f) == st.CLASS_SURFACE for f in AER)
    D = run_context(wide, (ncells, idx, w, series), graph)
    D.run(DT, steps, st.RUN_AEROSOL)
    want = aerosol.interpolate(series, last["month1"], last["month2"], last["month_wt1"], last["month_wt2"], idx, w)
    earlier = aerosol.interpolate(series, steps[-2]["month1"], steps[-2]["month2"], steps[-2]["month_wt1"], steps[-2]["month_wt2"], idx, w)
    got = state_of(D)
    for s in aerosol.STREAMS:
        assert same(got["aer_" + s], stored(D, want[s])), (kind, graph, s)
    D.close()
    assert not same(want["dst1_1"], earlier["dst1_1"]) and want["dst1_1"].any()
    # the run differed from the run without the flag: there aer_* stay what was uploaded
    cols = wide[0]
    for f in AER:
        assert same(wide_unflagged[f], np.ascontiguousarray(cols[f], dtype=np.float64)), f
        assert not same(got[f], wide_unflagged[f]), f


# ---- 3. against a second device path --------------------------------------------------------------------------------------------------
def test_deposition_equals_upload_gridded_of_host_interpolated_cells(base):
    """A single-term map of weight 1: elmk_upload_gridded of wt1 * x[m1] + wt2 * x[m2] formed on the host remaps the same numbers."""
    cols, scal, soil, lat, lon, _ = base
    nlon, nlat = 4, 3
    idx, w = regrid.nearest_map(np.degrees(lat), np.degrees(lon), nlon, nlat)
    ncells = nlon * nlat
    assert len(np.unique(idx)) > 3
    series = aerosol.synthetic_climatology(ncells, seed=11)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    reserve_and_upload(D, ncells, idx, w, series, months=(11, 0))
    D.aerosol_deposition(11, 0, 0.3, 0.7)
    first = D["aer_bcphi"]
    D.set_forcing_grid(idx, w, ncells)
    D.fill("aer_bcphi", -1.0)
    D.upload_gridded("aer_bcphi", 0.3 * series["bcphi"][11] + 0.7 * series["bcphi"][0])
    assert same(first, D["aer_bcphi"]) and first.any()
    D.close()


# ---- 4. the flag beside the others ----------------------------------------------------------------------------------------------------
def test_history_accum_and_aerosol_flags_together(base, mapped):
    cols, scal, soil, lat, lon, rec = base
    steps = schedule()
    out = []
    for run in (False, True):
        D = run_context(base, mapped, run)
        e = accum.add_t10(D, DT, period=4)
        ids = [D.history_add(0, "mss_dst1", "avg"), D.history_add(0, "aer_dst1_1", "max"), D.history_add(1, "t10", "avg")]
        if run:
            D.run(DT, steps, st.RUN_HISTORY | st.RUN_ACCUM | st.RUN_AEROSOL)
        else:
            stepwise_device(D, rec, steps, history=True, update_accum=True)
        out.append(([D.history_read(i) for i in ids], D.accum_read(e), D.history_count(0), state_of(D)))
        D.close()
    (ha, aa, ca, sa), (hb, ab, cb, sb) = out
    assert all(same(x, y) for x, y in zip(ha, hb)) and same(aa[0], ab[0]) and aa[1] == ab[1] == NSTEPS and ca == cb == NSTEPS
    assert_states(sa, sb)
    assert len(np.unique(hb[1])) > 2  # the deposition the tape saw


# ---- 5. restart -----------------------------------------------------------------------------------------------------------------------
def test_restart_in_the_middle_of_a_flagged_run(base, mapped, flagged):
    steps = schedule()
    half = NSTEPS // 2
    B = run_context(base, mapped, True)
    B.run(DT, steps[:half], st.RUN_AEROSOL)
    img = B.restart_save()
    B.close()
    D = run_context(base, None, True)
    for name, (fid, nlev, dt) in D.fields.items():
        D.fill(name, np.nan if dt == np.float64 else 3.0)
    D.restart_load(img)
    reserve_and_upload(D, *mapped)  # the series are an input: not in the image
    D.run(DT, steps[half:], st.RUN_AEROSOL)
    want = flagged[1]
    held = [k for k in want if st.field_class(k) in (st.CLASS_PROGNOSTIC, st.CLASS_SURFACE)]  # what an image holds
    for k in held:
        assert same(D[k], want[k]), k
    # the comparison covers the deposition's path: the eleven streams, the snow aerosol masses they grow and the snow mesh
    assert set(AER) <= set(held) and {"mss_dst1", "mss_bcphi", "snl", "h2osno", "t_soisno", "snw_rds"} <= set(held)
    assert all(st.field_class(f) == st.CLASS_SURFACE for f in AER)
    D.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(base, mapped, flagged):
    cols, scal, soil, lat, lon, rec = base
    ncells, idx, w, series = mapped
    steps = schedule()
    want_rows, want_state = flagged
    B = run_context(base, None, True)
    B.snapshot_fields(list(B.fields))
    lib, ctx = B.lib, B.ctx
    fid = B.fields["aer_bcphi"][0]
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    sa = np.ascontiguousarray(steps, dtype=st.RUN_STEP_DTYPE)
    month = np.ascontiguousarray(series["bcphi"][0])
    run_flagged = lambda: lib.elmk_run(ctx, DT, P(sa), int(sa.size), st.RUN_AEROSOL)  # noqa: E731

    def valid_run_still_gives_the_bits(what):
        B.restore_fields()
        B.run(DT, steps, st.RUN_AEROSOL)
        for g, wnt in zip(B.run_diagnostics(), want_rows):
            assert same(g, wnt), what
        assert_states(want_state, state_of(B), what)

    # without a reservation
    assert run_flagged() == -1
    assert lib.elmk_aerosol_deposition(ctx, 0, 1, 0.5, 0.5) == -1
    assert lib.elmk_aerosol_upload(ctx, fid, 0, 1, P(month)) == -1
    assert B.run_diagnostics()[0].shape == (0, 8, 3)  # no run was ever enqueued
    reserve_and_upload(B, ncells, idx, w, series)
    valid_run_still_gives_the_bits("no reservation")
    bytes1 = B.device_bytes

    # elmk_aerosol_reserve: every one leaves the reservation that exists as it is
    def bad_map(k, c, i=None, wt=None):
        ii, ww = idx.copy(), w.copy()
        if i is not None:
            ii[k, c] = i
        if wt is not None:
            ww[k, c] = wt
        return ncells, 3, P(ii), P(ww), (ii, ww)

    assert idx[1, 3] >= 0
    reserve_cases = {"idx[0] = -1": bad_map(0, 5, -1), "idx[0] = ncells": bad_map(0, 5, ncells), "idx[1] = -2": bad_map(1, 5, -2),
                     "idx[2] = ncells": bad_map(2, 5, ncells), "nan weight": bad_map(1, 3, None, np.nan), "inf weight": bad_map(0, 7, None, np.inf),
                     "npts 0": (ncells, 0, P(idx), P(w)), "npts 9": (ncells, 9, P(idx), P(w)), "ncells 0": (0, 3, P(idx), P(w)),
                     "ncells 2^31": (1 << 31, 3, P(idx), P(w)), "idx without w": (ncells, 3, P(idx), None), "w without idx": (ncells, 3, None, P(w)),
                     "no map and ncells != ncols": (ncells, 0, None, None)}
    for what, a in reserve_cases.items():
        assert lib.elmk_aerosol_reserve(ctx, *a[:4]) == -1, what
        assert B.device_bytes == bytes1, what
        valid_run_still_gives_the_bits(what)
    assert lib.elmk_aerosol_reserve(ctx, *reserve_cases["idx[0] = ncells"][:4]) == -1
    assert lib.elmk_last_error(ctx) == b"elmk_aerosol_reserve: idx[0] outside [0, ncells)"
    dep_cases = {"month1 -1": (-1, 0, 0.5, 0.5), "month1 12": (12, 0, 0.5, 0.5), "month2 -1": (0, -1, 0.5, 0.5), "month2 12": (0, 12, 0.5, 0.5),
                 "wt1 nan": (0, 1, np.nan, 0.5), "wt2 inf": (0, 1, 0.5, np.inf), "wt1 -inf": (0, 1, -np.inf, 0.5)}
    for what, a in dep_cases.items():
        assert lib.elmk_aerosol_deposition(ctx, *a) == -1, what
        valid_run_still_gives_the_bits(what)
    up_cases = {"field before the eleven": (fid - 1, 0, 1), "field after the eleven": (fid + 11, 0, 1), "field -1": (-1, 0, 1),
                "month0 -1": (fid, -1, 1), "nmonths 0": (fid, 0, 0), "nmonths -1": (fid, 3, -1), "month0 + nmonths 13": (fid, 12, 1),
                "past December": (fid, 6, 7)}
    big = np.full((13, ncells), 1.0e30)
    for what, a in up_cases.items():
        assert lib.elmk_aerosol_upload(ctx, a[0], a[1], a[2], P(big)) == -1, what
        valid_run_still_gives_the_bits(what)
    assert lib.elmk_aerosol_upload(ctx, fid, 0, 1, None) == -1
    s = steps.copy()
    s[7]["month2"] = 12
    s = np.ascontiguousarray(s, dtype=st.RUN_STEP_DTYPE)
    assert lib.elmk_run(ctx, DT, P(s), int(s.size), st.RUN_AEROSOL) == -1
    assert lib.elmk_run(ctx, DT, P(sa), int(sa.size), 16) == -1  # the next flag bit does not exist
    valid_run_still_gives_the_bits("bad run")
    # a stream being captured
    with captured(B):
        rcs = [lib.elmk_aerosol_reserve(ctx, ncells, 3, P(idx), P(w)), lib.elmk_aerosol_upload(ctx, fid, 0, 1, P(month)),
               lib.elmk_aerosol_deposition(ctx, 0, 1, 0.5, 0.5), lib.elmk_aerosol_clear(ctx), run_flagged()]
    assert rcs == [-1] * 5, rcs
    assert B.device_bytes == bytes1
    valid_run_still_gives_the_bits("stream being captured")

    # an upload enqueued right after a run that reads the series waits for it (it cannot be forced to race; an upload that did not
    # wait would most likely land under the run's later steps)
    B.restore_fields()
    B.run(DT, steps, st.RUN_AEROSOL)
    for sname in aerosol.STREAMS:
        B.aerosol_upload(sname, 0, big[:2])
        B.aerosol_upload(sname, 11, big[0])
    for g, wnt in zip(B.run_diagnostics(), want_rows):
        assert same(g, wnt)
    assert_states(want_state, state_of(B), "upload behind a run")

    # a new reservation between two runs under the graph: the captured step of the old one is dropped, not replayed
    ncells2, idx2, w2 = make_map("n1", N, ncells=5, seed=17)
    series2 = aerosol.synthetic_climatology(ncells2, seed=19)
    W = run_context(base, (ncells2, idx2, w2, series2), False)
    W.run(DT, steps, st.RUN_AEROSOL)
    rows2, state2 = W.run_diagnostics(), state_of(W)
    W.close()
    assert not same(state2["mss_dst1"], want_state["mss_dst1"])
    reserve_and_upload(B, ncells2, idx2, w2, series2)
    B.restore_fields()
    B.run(DT, steps, st.RUN_AEROSOL)
    for g, wnt in zip(B.run_diagnostics(), rows2):
        assert same(g, wnt)
    assert_states(state2, state_of(B), "reserve between two runs")
    # ... and a clear: the flag is refused again, the unflagged run is the run of a context that never had a series
    W = run_context(base, None, False)
    W.run(DT, steps)
    rows3, state3 = W.run_diagnostics(), state_of(W)
    W.close()
    bytes0 = bytes1 - expected_bytes(B, ncells, idx)
    B.aerosol_clear()
    assert B.device_bytes == bytes0
    assert run_flagged() == -1
    B.restore_fields()
    B.run(DT, steps)
    for g, wnt in zip(B.run_diagnostics(), rows3):
        assert same(g, wnt)
    assert_states(state3, state_of(B), "clear between two runs")
    for f in AER:
        assert same(B[f], np.ascontiguousarray(cols[f], dtype=np.float64)), f
    B.close()


# ---- 7. the demo ----------------------------------------------------------------------------------------------------------------------
def test_aerosol_demo(tmp_path):
    """examples/aerosol_demo.cc builds against the C ABI and runs 48 steps across a month boundary against the stepwise loop."""
    n = 320
    cols, scal, soil, lat, lon, rec = _inputs(n, SEED, nrec=25)
    exe = build_demo("aerosol_demo", tmp_path)
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, demo_records(lat, lon, rec) + [("steps", schedule(48))]))
    r = run_demo(exe, tmp_path / "state.bin")
    assert "bit-identical" in r.stdout and "mss_dst1 of column" in r.stdout, r.stdout
