"""Forcing on a coarser grid (include/elmk.h "forcing grid"): every device remap is compared bit for bit with the same records remapped
on the host by regrid.apply_map and sent per column through the existing calls - elmk_upload for the stepwise path, per-column series
for elmk_run."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests import helpers as H
from tests import run_cases as GR
from tests.support import build_demo, captured, run_demo, same, state_blob

pytestmark = pytest.mark.gpu

DT, NREC, NSTEPS = GR.DT, GR.NREC, GR.NSTEPS
NLON, NLAT = 64, 32
NCELLS = NLON * NLAT


def _cell_records(ncells, seed, nrec=NREC):
    """Forcing records on the cells, [nrec, ncells] per atm_* stream, with the ranges and branches of run_cases' records."""
    return {k: v for k, v in GR._inputs(ncells, seed, nrec=nrec)[-1].items() if k in st.SERIES_FORCING}


def _map(kind, lat_r, lon_r, seed=0):
    """(idx, w) of one kind of map from the columns' geography (radians) to the NLON x NLAT grid."""
    lat, lon = np.degrees(lat_r), np.degrees(lon_r)
    if kind == "nearest":
        return RG.nearest_map(lat, lon, NLON, NLAT)
    if kind == "bilinear":
        return RG.bilinear_map(lat, lon, NLON, NLAT)
    if kind == "bilinear_land":
        land = np.random.default_rng(seed).random(NCELLS) < 0.6
        return RG.bilinear_map(lat, lon, NLON, NLAT, land=land)
    # "sparse<m>": a map file's triplets, 1 .. m distinct cells per column around the nearest one (padding where fewer)
    m = int(kind[6:])
    n = lat.size
    rng = np.random.default_rng(seed)
    near = RG.nearest_map(lat, lon, NLON, NLAT)[0][0].astype(np.int64)
    cnt = rng.integers(1, m + 1, n)
    row = np.repeat(np.arange(n), cnt)
    off = np.concatenate([np.arange(c) for c in cnt])
    col = (near[row] + off * 37) % NCELLS
    S = rng.random(row.size) + 0.05
    S = S / np.bincount(row, S)[row]
    perm = rng.permutation(row.size)  # a map file lists its triplets in any order
    return RG.from_sparse(row[perm], col[perm], S[perm], n, NCELLS)


def _column_records(idx, w, cells, rec):
    """The per-column series of a grid run: forcing = the host remap of every cell record, phenology as it is."""
    out = dict(rec)
    for k in st.SERIES_FORCING:
        out[k] = RG.apply_map(idx, w, cells[k])
    return out


@pytest.fixture(scope="module")
def base():
    cols, scal, soil, lat, lon, rec = GR._inputs(5003, 81)
    return cols, scal, soil, lat, lon, rec, _cell_records(NCELLS, 82)


def _grid_run(B, idx, w, cells, rec, steps, slots=NREC):
    B.set_forcing_grid(idx, w, NCELLS)
    B.run_reserve(slots, len(steps))
    for k in st.SERIES_FORCING:
        B.series_upload(k, 0, cells[k])
    for k in st.SERIES_PHENOLOGY:
        B.series_upload(k, 0, rec[k])
    B.run(DT, steps)
    return B.run_diagnostics()


def _column_run(A, rec_cols, steps, slots=NREC):
    A.run_reserve(slots, len(steps))
    GR.upload_series(A, rec_cols)
    A.run(DT, steps)
    return A.run_diagnostics()


def _assert_same_state(A, B, skip=()):
    for name in A.fields:
        if name not in skip:
            assert same(A[name], B[name]), name


@pytest.mark.parametrize("lib", ["f64", "f32"])
def test_upload_gridded_equals_upload_of_the_host_remap(base, lib):
    """Both levels of every atm_*, an aer_* field and one level of a multi-level field."""
    cols, scal, soil, lat, lon, rec, cells = base
    path = L.F32_LIB_PATH if lib == "f32" else None
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=path)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=path)
    idx, w = _map("bilinear_land", lat, lon, 3)
    B.set_forcing_grid(idx, w, NCELLS)
    rng = np.random.default_rng(83)
    jobs = [(k, lev, cells[k][3 + lev]) for k in st.SERIES_FORCING for lev in (0, 1)]
    jobs += [("aer_dst2_1", 0, rng.random(NCELLS) * 1e-9), ("t_soisno", 7, 250.0 + 40.0 * rng.random(NCELLS))]
    for name, lev, c in jobs:
        B.upload_gridded(name, c, level=lev)
        full = A[name]
        v = RG.apply_map(idx, w, c)
        if full.ndim == 1:
            full = v
        else:
            full[:, lev] = v
        A.upload(name, full)
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_twelve_stepwise_steps_with_gridded_uploads(base):
    """The stepwise driver's path: 12 steps whose forcing goes up with upload_gridded equal 12 steps whose forcing goes up as the host
    remap, in every field."""
    cols, scal, soil, lat, lon, rec, cells = base
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    idx, w = _map("bilinear", lat, lon)
    B.set_forcing_grid(idx, w, NCELLS)
    rec_cols = _column_records(idx, w, cells, rec)
    steps = GR.schedule()
    for D, gridded in ((A, False), (B, True)):
        D.set_graph(True)
        for p in steps:
            D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
            f = int(p["forc_slot"])
            for k in st.SERIES_FORCING:
                if gridded:
                    D.upload_gridded(k, cells[k][f], level=0)
                    D.upload_gridded(k, cells[k][f + 1], level=1)
                else:
                    D.upload(k, np.stack([rec_cols[k][f], rec_cols[k][f + 1]], axis=1))
            for k in st.SERIES_PHENOLOGY:
                D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
            st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
            st.get_forcing(D, p["forc_wt1"], p["forc_wt2"])
            st.kokkos_init_timestep(D)
            st.advance_physics(D, DT)
    _assert_same_state(A, B)
    assert not same(A["forc_tbot"], cols["forc_tbot"])
    A.close()
    B.close()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("kind", ["nearest", "sparse2", "bilinear", "sparse3", "sparse7"])
def test_grid_run_equals_per_column_run(base, kind, graph):
    """A run over cell records equals the run over per-column series equal to apply_map of each record: npts 1, 2, 4 (bilinear, and
    3 terms padded to 4 with -1), 7 padded to 8."""
    cols, scal, soil, lat, lon, rec, cells = base
    A, B = GR._pair(base[:6], graph=graph)
    idx, w = _map(kind, lat, lon, 5)
    if kind.startswith("sparse"):
        assert np.any(idx < 0) and idx.shape[0] == int(kind[6:])
    steps = GR.schedule()
    want = _column_run(A, _column_records(idx, w, cells, rec), steps)
    got = _grid_run(B, idx, w, cells, rec, steps)
    GR.assert_same_rows(got, want)
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_two_runs_with_a_cell_window_between_equal_one_run(base):
    """5 + 7 steps: the cell records of the second window (slots 4 ..) go up while the first run (slots 0 .. 3) is in flight."""
    cols, scal, soil, lat, lon, rec, cells = base
    A, B = GR._pair(base[:6])
    idx, w = _map("bilinear", lat, lon)
    steps = GR.schedule()
    want = _grid_run(A, idx, w, cells, rec, steps)
    B.set_forcing_grid(idx, w, NCELLS)
    B.run_reserve(NREC, 8)
    for k in st.SERIES_FORCING:
        B.series_upload(k, 0, cells[k][0:4])
    for k in st.SERIES_PHENOLOGY:
        B.series_upload(k, 0, rec[k])
    B.run(DT, steps[:5])
    for k in st.SERIES_FORCING:
        B.series_upload(k, 4, cells[k][4:NREC])
    B.run(DT, steps[5:])
    GR.assert_same_rows(B.run_diagnostics(), tuple(x[5:] for x in want))
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_large_launch_grid_run():
    """262 144 columns (the benchmark's launch structure), bilinear map, three steps."""
    cols, scal, soil, lat, lon, rec = GR._inputs(262144, 84)
    cells = _cell_records(NCELLS, 85)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    for D in (A, B):
        D.set_graph(True)
    idx, w = _map("bilinear", lat, lon)
    steps = GR.schedule(3)
    want = _column_run(A, _column_records(idx, w, cells, rec), steps)
    GR.assert_same_rows(_grid_run(B, idx, w, cells, rec, steps), want)
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_refusals_enqueue_nothing(base):
    """Every refusal returns ELMK_E_INVALID and changes nothing: the reservation, the series and the map stay, and a valid run from
    the same start still gives the bits."""
    cols, scal, soil, lat, lon, rec, cells = base
    A, B = GR._pair(base[:6])
    idx, w = _map("sparse3", lat, lon, 6)
    steps = GR.schedule()
    want = _column_run(A, _column_records(idx, w, cells, rec), steps)
    want_state = {name: A[name] for name in A.fields if name not in GR.SERIES}
    B.snapshot_fields(list(B.fields))
    lib, ctx, n = B.lib, B.ctx, B.ncols
    assert lib.elmk_upload_gridded(ctx, B.fields["atm_tbot"][0], 0, cells["atm_tbot"][0].ctypes.data_as(C.c_void_p)) == -1  # no map
    _grid_run(B, idx, w, cells, rec, steps)

    def still_gives_the_bits(what):
        B.restore_fields()
        B.run(DT, steps)
        GR.assert_same_rows(B.run_diagnostics(), want)
        for name, v in want_state.items():
            assert same(B[name], v), (what, name)

    def set_refused(i, ww, ncells=NCELLS, npts=None):
        i = np.ascontiguousarray(i, np.int32)
        ww = np.ascontiguousarray(ww, np.float64)
        return lib.elmk_set_forcing_grid(ctx, int(ncells), int(i.shape[0] if npts is None else npts), i.ctypes.data_as(C.c_void_p),
                                         ww.ctypes.data_as(C.c_void_p)) == -1

    pad = np.nonzero(idx[1] < 0)[0][0]  # a column with padding in row 1
    cases = [("npts 0", idx, w, NCELLS, 0), ("npts 9", np.vstack([idx] * 3)[:9], np.vstack([w] * 3)[:9], NCELLS, 9),
             ("ncells 0", idx, w, 0, None), ("ncells 2^31", idx, w, 1 << 31, None)]
    for what, k, c, v in (("idx[0] -1", 0, 17, -1), ("idx[0] ncells", 0, 17, NCELLS), ("idx[1] -2", 1, 17, -2),
                          ("idx[2] ncells", 2, 17, NCELLS)):
        i = idx.copy()
        i[k, c] = v
        cases.append((what, i, w, NCELLS, None))
    for what, x in (("w nan", np.nan), ("w inf", np.inf)):
        ww = w.copy()
        ww[0, 23] = x
        cases.append((what, idx, ww, NCELLS, None))
    for what, i, ww, nc, npts in cases:
        assert set_refused(i, ww, nc, npts), what
        still_gives_the_bits(what)
    assert cases[-1][0] == "w inf" and lib.elmk_last_error(ctx) == b"elmk_set_forcing_grid: non-finite weight"
    assert cases[6][0] == "idx[1] -2" and set_refused(*cases[6][1:])
    assert lib.elmk_last_error(ctx) == b"elmk_set_forcing_grid: idx outside [-1, ncells)"
    for what, f, lev in (("int field", B.fields["snl"][0], 0), ("level 2", B.fields["atm_tbot"][0], 2), ("level -1", B.fields["atm_tbot"][0], -1),
                         ("unknown field", 100000, 0)):
        assert lib.elmk_upload_gridded(ctx, f, lev, cells["atm_tbot"][0].ctypes.data_as(C.c_void_p)) == -1, what
        still_gives_the_bits(what)
    # a stream being captured: set, clear and upload_gridded refuse
    with captured(B):
        rcs = [lib.elmk_set_forcing_grid(ctx, NCELLS, idx.shape[0], np.ascontiguousarray(idx, np.int32).ctypes.data_as(C.c_void_p),
                                         np.ascontiguousarray(w).ctypes.data_as(C.c_void_p)),
               lib.elmk_clear_forcing_grid(ctx),
               lib.elmk_upload_gridded(ctx, B.fields["atm_tbot"][0], 0, cells["atm_tbot"][0].ctypes.data_as(C.c_void_p))]
    assert rcs == [-1, -1, -1]
    still_gives_the_bits("stream being captured")
    # a non-finite weight behind padding is accepted (never read), and the run still gives the bits
    ww = w.copy()
    ww[1, pad] = np.nan
    B.set_forcing_grid(idx, ww, NCELLS)
    B.restore_fields()
    GR.assert_same_rows(_grid_run(B, idx, ww, cells, rec, steps), want)
    A.close()
    B.close()


def test_set_and_clear_release_the_reservation(base):
    cols, scal, soil, lat, lon, rec, cells = base
    A, B = GR._pair(base[:6])
    idx, w = _map("nearest", lat, lon)
    steps = GR.schedule()

    def run_refused():
        a = np.ascontiguousarray(steps, dtype=st.RUN_STEP_DTYPE)
        return B.lib.elmk_run(B.ctx, DT, a.ctypes.data_as(C.c_void_p), int(a.size), 0) == -1

    B.run_reserve(NREC, NSTEPS)
    GR.upload_series(B, rec)
    B.set_forcing_grid(idx, w, NCELLS)
    assert run_refused()
    with pytest.raises(L.ElmkError):
        B.series_upload("atm_tbot", 0, cells["atm_tbot"])
    B.run_reserve(NREC, NSTEPS)
    B.set_forcing_grid(idx, w, NCELLS)  # replacing the map releases too
    assert run_refused()
    B.run_reserve(NREC, NSTEPS)
    with pytest.raises(L.ElmkError):  # cell records: n is checked against ncells
        B.series_upload("atm_tbot", 0, np.zeros((1, NCELLS + 1)))
    B.series_upload("mlai", 0, rec["mlai"])  # phenology stays per column
    B.clear_forcing_grid()
    assert run_refused()
    # after clear: per-column runs as in a context that never had a map
    want = _column_run(A, rec, steps)
    GR.assert_same_rows(_column_run(B, rec, steps), want)
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_device_bytes_account_for_the_map_and_the_cell_series(base):
    cols, scal, soil, lat, lon, rec, cells = base
    D = GR.device(base)
    ld, es = D.level_stride, D.lib.elmk_state_real_bytes()

    def al(b):
        return (b + 255) // 256 * 256

    b0 = D.device_bytes
    idx, w = _map("sparse3", lat, lon, 7)  # npts 3: stored as 4 rows
    D.set_forcing_grid(idx, w, NCELLS)
    assert D.device_bytes - b0 == al(4 * ld * 4) + al(4 * ld * 8) + al(NCELLS * 8)
    b1 = D.device_bytes
    slots, msteps = 25, 48
    D.run_reserve(slots, msteps)
    grid_run = D.device_bytes - b1
    D.clear_forcing_grid()
    assert D.device_bytes == b0
    D.run_reserve(slots, msteps)
    col_run = D.device_bytes - b0
    assert col_run - grid_run == al(7 * slots * ld * es) - al(7 * slots * NCELLS * es)
    D.close()


def test_fp32_build_nearest_map_is_bitwise():
    """libelmk_f32.so stores the cell records as fp32; with one term of weight 1.0 per column the remap is exact, so a grid run
    equals the per-column run bit for bit."""
    cols, scal, soil, lat, lon, rec = GR._inputs(2053, 86)
    cells = _cell_records(NCELLS, 87)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=L.F32_LIB_PATH)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=L.F32_LIB_PATH)
    assert B.lib.elmk_state_real_bytes() == 4
    idx, w = _map("nearest", lat, lon)
    steps = GR.schedule()
    want = _column_run(A, _column_records(idx, w, cells, rec), steps)
    GR.assert_same_rows(_grid_run(B, idx, w, cells, rec, steps), want)
    _assert_same_state(A, B)
    A.close()
    B.close()


def test_forcing_grid_demo(tmp_path):
    """examples/forcing_grid_demo.cc: a global grid of columns forced from 64 x 32 cells for a day of 48 steps as two runs; its
    PrimaryVars and conservation rows equal the Python layer's stepwise run with upload_gridded."""
    n, nsteps, nrec = 3008, 48, 25
    cols, scal, soil, lat, lon, rec = GR._inputs(n, 88, nrec=nrec)
    cells = _cell_records(NCELLS, 89, nrec=nrec)
    steps = GR.schedule(nsteps)
    exe = build_demo("forcing_grid_demo", tmp_path)
    idx, w = _map("bilinear", lat, lon)
    extra = [("lat", lat), ("lon", lon)] + [(f"cells/{k}", np.ascontiguousarray(cells[k], np.float64)) for k in st.SERIES_FORCING]
    extra += [(f"series/{k}", np.ascontiguousarray(rec[k], np.float64)) for k in st.SERIES_PHENOLOGY]
    extra += [("map/idx", idx.astype(np.int32)), ("map/w", w), ("steps", steps)]
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, extra))
    r = run_demo(exe, tmp_path / "state.bin", tmp_path / "out.bin")
    assert "48 steps" in r.stdout and "2048 forcing cells (4 terms per column)" in r.stdout, r.stdout
    # the same steps through the Python layer, stepwise with upload_gridded
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_graph(True)
    D.set_forcing_grid(idx, w, NCELLS)
    cons = []
    for p in steps:
        D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
        f = int(p["forc_slot"])
        for k in st.SERIES_FORCING:
            D.upload_gridded(k, cells[k][f], level=0)
            D.upload_gridded(k, cells[k][f + 1], level=1)
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"])
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        cons.append(st.kokkos_evaluate_conservation(D, DT))
    raw = (tmp_path / "out.bin").read_bytes()
    off = 0
    for name in st.ELMInterface.PRIMARY_VARS:
        want = D[name]
        got = np.frombuffer(raw, want.dtype, want.size, off).reshape(want.shape)
        off += want.nbytes
        assert same(got, want), name
    got = np.frombuffer(raw, np.float64, nsteps * 24, off).reshape(nsteps, 8, 3)
    assert same(got, np.array(cons))
    assert off + nsteps * 24 * 8 == len(raw)
    D.close()
