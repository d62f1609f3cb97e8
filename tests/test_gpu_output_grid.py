"""Output on a grid (include/elmk.h "output grid"): every device aggregate is compared bit for bit with regrid.apply_aggregate of the same
fields taken with elmk_download - gridded downloads, gridded history tapes stepwise and through elmk_run, tapes that mix column and
gridded entries, a caller's graph, the refusals, the device memory, libelmk_f32.so and the example."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests import helpers as H
from tests import run_cases as GR
from tests.output_map_cases import CellTapes, host_aggregate
from tests.support import build_demo, captured, run_demo, same_nan, state_blob

pytestmark = pytest.mark.gpu

DT, NREC, NSTEPS = GR.DT, GR.NREC, GR.NSTEPS
FILL = 1.0e36  # ELM's spval
# one level of every stored type: F64 (one level and every level of a 20-level field), I32, U8, U32
FIELDS = ["t_grnd", "eflx_sh_tot", "t_soisno", "snl", "veg_active", "err_flags"]


def _levels(D, name):
    return D.fields[name][1]


def owner(ncols, ncells, seed, shuffled=False, big=0):
    """An ownership map with cell-contiguous columns (shuffled=True: the same cells, columns permuted).  Every fifth cell, the first
    and the last are empty; big > 0 gives cell 3 that many columns."""
    rng = np.random.default_rng(seed)
    live = np.array([c for c in range(1, ncells - 1) if c % 5])
    cell = np.sort(rng.choice(live, ncols))
    if big:
        cell[ncols // 3:ncols // 3 + big] = 3
        cell = np.sort(cell)
    if shuffled:
        cell = cell[rng.permutation(ncols)]
    area = rng.random(ncols) * 2.0 + 0.05
    return RG.owner_map(cell, area, ncells)


def triplets(ncols, ncells, seed):
    """A land -> atmosphere map file's triplets: 0 .. 6 terms per cell over any columns (repeats included), in file order."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 7, ncells)
    row = np.repeat(np.arange(ncells), cnt)
    col = rng.integers(0, ncols, row.size)
    S = rng.random(row.size) * 0.4
    perm = rng.permutation(row.size)
    return RG.from_sparse_cells(row[perm], col[perm], S[perm], ncells, ncols)


@pytest.fixture(scope="module")
def stepped():
    """A 5003-column context after one model step (ncols not a multiple of 64)."""
    cols, scal, soil, lat, lon, rec = GR._inputs(5003, 91)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    GR.stepwise(D, rec, GR.schedule(1))
    yield D
    D.close()


MAPS = {
    "owner_sorted": lambda n: owner(n, 211, 1),
    "owner_shuffled": lambda n: owner(n, 211, 1, shuffled=True),
    "triplets": lambda n: triplets(n, 300, 2),
    "big_cell": lambda n: owner(n, 40, 3, shuffled=True, big=1500),
}


@pytest.mark.parametrize("kind", sorted(MAPS))
def test_download_gridded_equals_the_host_aggregate(stepped, kind):
    D = stepped
    ptr, col, w = MAPS[kind](D.ncols)
    D.set_output_grid(ptr, col, w, FILL)
    if kind == "big_cell":
        assert ptr[4] - ptr[3] > 1000
    assert np.any(np.diff(ptr) == 0)  # empty cells
    for name in FIELDS:
        want = host_aggregate(D, name, ptr, col, w)
        for lev in range(_levels(D, name)):
            got = D.download_gridded(name, level=lev)
            assert same_nan(got, want if want.ndim == 1 else want[:, lev]), (kind, name, lev)
    assert np.all(D.download_gridded("t_grnd")[np.diff(ptr) == 0] == FILL)


def test_one_column_and_cells_past_the_staging_chunk():
    """ncols = 1 with more cells than the staging buffer holds at once (chunked download), and a 1-cell map."""
    D = st.ELMState(1)
    D["t_grnd"] = np.array([271.25])
    D["snl"] = np.array([3], np.int32)
    ncells = 5000
    ptr = np.zeros(ncells + 1, np.int64)
    ptr[1:] = np.cumsum(np.arange(ncells) % 3 == 1)  # one term in every third cell
    nnz = int(ptr[-1])
    D.set_output_grid(ptr, np.zeros(nnz, np.int32), np.linspace(0.5, 1.5, nnz), -0.0)
    for name in ("t_grnd", "snl"):
        assert same_nan(D.download_gridded(name), host_aggregate(D, name, ptr, np.zeros(nnz, np.int32), np.linspace(0.5, 1.5, nnz), -0.0))
    D.set_output_grid([0, 2], [0, 0], [0.25, 0.75], FILL)
    assert same_nan(D.download_gridded("t_grnd"), [0.25 * 271.25 + 0.75 * 271.25])
    D.close()


def test_four_million_columns():
    """2^22 + 37 columns on a 0.5-degree-like grid (~67 k cells), shuffled, for the 64-bit offsets of the map and the sources."""
    n = (1 << 22) + 37
    D = st.ELMState(n)
    rng = np.random.default_rng(5)
    t = 250.0 + 60.0 * rng.random((n, _levels(D, "t_soisno")))
    D["t_soisno"] = t
    D["snl"] = rng.integers(0, 6, n).astype(np.int32)
    ptr, col, w = owner(n, 67420, 6, shuffled=True)
    D.set_output_grid(ptr, col, w, FILL)
    for lev in (0, 19):
        assert same_nan(D.download_gridded("t_soisno", level=lev), RG.apply_aggregate(ptr, col, w, t[:, lev], FILL)), lev
    assert same_nan(D.download_gridded("snl"), host_aggregate(D, "snl", ptr, col, w))
    D.close()


# (tape, field, op): every op on F64 with one level and with 20 levels, I32 and U8; tape 3 has gridded entries only
GRIDDED = [(0, "t_grnd", "avg"), (0, "t_soisno", "avg"), (0, "snl", "avg"), (1, "t_grnd", "max"), (1, "h2osoi_liq", "min"),
           (1, "veg_active", "sum"), (2, "eflx_sh_tot", "sum"), (2, "snl", "inst"), (3, "t_grnd", "min"), (3, "eflx_sh_tot", "avg"),
           (3, "h2osoi_liq", "max"), (3, "qflx_evap_tot", "inst")]
COLUMN = [(0, "t_grnd", "avg"), (1, "h2osoi_liq", "max"), (2, "snl", "inst"), (2, "eflx_sh_tot", "sum")]


def _add(D, gridded, column):
    g = [D.gridded_history_add(t, f, op) for t, f, op in gridded]
    c = [D.history_add(t, f, op) for t, f, op in column]
    return g, c


@pytest.mark.parametrize("graph", [False, True])
def test_gridded_history_stepwise_and_run_equal_the_host_fold(graph):
    """A (stepwise, history_accumulate after every step) against the host fold of the aggregates of A's downloads; B (elmk_run with
    ELMK_RUN_HISTORY) gives the same bits; C (the column entries alone, through elmk_run) gives B's column entries their bits."""
    cols, scal, soil, lat, lon, rec = base = GR._inputs(5003, 93)
    A, B = GR._pair(base, graph=graph)
    Cc = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    Cc.set_graph(graph)
    ptr, col, w = owner(A.ncols, 157, 7, shuffled=True)
    empty = np.diff(ptr) == 0
    for D in (A, B):
        D.set_output_grid(ptr, col, w, FILL)
    ids = {D: _add(D, GRIDDED, COLUMN) for D in (A, B)}
    _, ids_c = _add(Cc, [], COLUMN)
    # gridded and column ids share one table, in order of registration
    assert ids[A][0] == list(range(len(GRIDDED))) and ids[A][1] == list(range(len(GRIDDED), len(GRIDDED) + len(COLUMN)))
    ref = CellTapes(GRIDDED, empty)
    names = sorted({f for _, f, _ in GRIDDED})
    steps = GR.schedule()
    for s in range(NSTEPS):
        GR.stepwise(A, rec, steps[s:s + 1], st.RUN_HISTORY)
        ref.fold({k: host_aggregate(A, k, ptr, col, w) for k in names})
    for D in (B, Cc):
        D.run_reserve(NREC, NSTEPS)
        GR.upload_series(D, rec)
        D.run(DT, steps, st.RUN_HISTORY)
    for k, (t, f, op) in enumerate(GRIDDED):
        want = ref.result(k)
        for D in (A, B):
            got = D.history_read(ids[D][0][k])
            assert same_nan(got, want), (D is B, t, f, op)
        if want.ndim == 2:
            c0, m = 11, 97
            assert same_nan(B.history_read(ids[B][0][k], col0=c0, n=m, layout=st.LAYOUT_SOA), want[c0:c0 + m].T), (t, f, op)
    for k in range(len(COLUMN)):
        want = Cc.history_read(ids_c[k])
        assert same_nan(A.history_read(ids[A][1][k]), want) and same_nan(B.history_read(ids[B][1][k]), want), COLUMN[k]
    for t in range(st.HIST_MAX_TAPES):
        assert A.history_count(t) == B.history_count(t) == NSTEPS, t  # tape 3: gridded entries only
    GR.assert_same_state(A, B, cols)
    # a new gridded entry after a reset: the captured run step is taken again with it
    B.history_reset(0)
    e = B.gridded_history_add(0, "t_grnd", "inst")
    B.run(DT, steps[:2], st.RUN_HISTORY)
    assert B.history_count(0) == 2 and B.history_count(3) == NSTEPS + 2
    assert same_nan(B.history_read(e), host_aggregate(B, "t_grnd", ptr, col, w))
    for D in (A, B, Cc):
        D.close()


def test_gridded_accumulate_inside_a_callers_graph():
    """history_accumulate with column and gridded entries captured into a caller's graph and replayed N times; set / clear of the
    output grid and download_gridded are refused while the stream is being captured."""
    n, N = 4099, 7
    D = st.ELMState(n)
    rng = np.random.default_rng(9)
    t = rng.standard_normal(n) * 300.0
    D["t_grnd"] = t
    ptr, col, w = owner(n, 90, 10)
    D.set_output_grid(ptr, col, w, FILL)
    eg = D.gridded_history_add(0, "t_grnd", "sum")
    ec = D.history_add(0, "t_grnd", "max")
    eo = D.gridded_history_add(1, "t_grnd", "avg")  # tape 1: gridded only
    with captured(D) as cap:
        rc_acc = D.lib.elmk_history_accumulate(D.ctx)
        p64 = np.ascontiguousarray(ptr)
        rc_set = D.lib.elmk_set_output_grid(D.ctx, p64.size - 1, p64.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                            w.ctypes.data_as(C.c_void_p), 0.0)
        rc_clr = D.lib.elmk_clear_output_grid(D.ctx)
        out = np.empty(p64.size - 1)
        rc_dl = D.lib.elmk_download_gridded(D.ctx, D.fields["t_grnd"][0], 0, out.ctypes.data_as(C.c_void_p))
        cap.end()
        assert rc_acc == 0 and rc_set == rc_clr == rc_dl == -1
        cap.replay(N)
        assert D.history_count(0) == N and D.history_count(1) == N
        g = RG.apply_aggregate(ptr, col, w, t, FILL)
        acc = np.full(g.shape, -0.0)
        for _ in range(N):
            acc = acc + g
        empty = np.diff(ptr) == 0
        assert same_nan(D.history_read(eg), np.where(empty, FILL, acc))
        assert same_nan(D.history_read(eo), np.where(empty, FILL, acc / float(N)))
        assert same_nan(D.history_read(ec), t)
    D.close()


def _set(D, ncells, ptr, col, w, fill=0.0):
    ptr = np.ascontiguousarray(ptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    return D.lib.elmk_set_output_grid(D.ctx, int(ncells), ptr.ctypes.data_as(C.c_void_p), col.ctypes.data_as(C.c_void_p),
                                      w.ctypes.data_as(C.c_void_p), float(fill))


def test_refusals_enqueue_nothing_and_leave_the_context_working():
    n = 777
    D = st.ELMState(n)
    x = np.random.default_rng(11).standard_normal(n)
    D["t_grnd"] = x
    fid = D.fields["t_grnd"][0]
    out = np.empty(4)
    # without a map
    assert D.lib.elmk_download_gridded(D.ctx, fid, 0, out.ctypes.data_as(C.c_void_p)) == -1
    assert D.lib.elmk_gridded_history_add(D.ctx, 0, fid, st.HIST_AVG) == -1
    ptr, col, w = np.array([0, 2, 2, 3, 5]), np.array([0, 5, 776, 3, 3]), np.array([0.5, 0.5, 1.0, 0.25, 0.75])
    D.set_output_grid(ptr, col, w, FILL)
    want = RG.apply_aggregate(ptr, col, w, x, FILL)
    assert same_nan(D.download_gridded("t_grnd"), want)
    bad = [(0, [0], [], []), (-3, ptr, col, w), (1 << 31, ptr, col, w),  # ncells
           (4, [1, 2, 2, 3, 5], col, w), (4, [0, 2, 1, 3, 5], col, w),  # ptr[0], decreasing
           (4, ptr, [0, 5, 777, 3, 3], w), (4, ptr, [0, -1, 7, 3, 3], w),  # col outside [0, ncols)
           (4, ptr, col, [0.5, np.nan, 1.0, 0.25, 0.75]), (4, ptr, col, [0.5, 0.5, np.inf, 0.25, 0.75])]  # weights
    for k, (nc, p, c, ww) in enumerate(bad):
        assert _set(D, nc, p, c, ww) == -1, k
        assert same_nan(D.download_gridded("t_grnd"), want), k  # the map in place is untouched
    assert np.isinf(bad[-1][3][2]) and D.lib.elmk_last_error(D.ctx) == b"elmk_set_output_grid: non-finite weight"
    assert list(bad[4][1]) == [0, 2, 1, 3, 5] and _set(D, *bad[4]) == -1
    assert D.lib.elmk_last_error(D.ctx) == b"elmk_set_output_grid: ptr decreasing"
    big = np.array([0, (1 << 31)], np.int64)  # nnz outside 0 .. 2^31-1 (refused before col / w are read)
    assert D.lib.elmk_set_output_grid(D.ctx, 1, big.ctypes.data_as(C.c_void_p), None, None, 0.0) == -1
    nf = D.lib.elmk_num_fields()
    for f, lev in ((-1, 0), (nf, 0), (fid, 1), (fid, -1), (D.fields["t_soisno"][0], _levels(D, "t_soisno"))):
        assert D.lib.elmk_download_gridded(D.ctx, f, lev, out.ctypes.data_as(C.c_void_p)) == -1, (f, lev)
    for tape, f, op in ((-1, fid, 0), (st.HIST_MAX_TAPES, fid, 0), (0, -1, 0), (0, nf, 0), (0, fid, 5)):
        assert D.lib.elmk_gridded_history_add(D.ctx, tape, f, op) == -1, (tape, f, op)
    # with a gridded entry: set and clear refused; without one again: allowed
    e = D.gridded_history_add(0, "t_grnd", "avg")
    D.history_accumulate()
    assert _set(D, 4, ptr, col, w) == -1 and D.lib.elmk_clear_output_grid(D.ctx) == -1
    assert same_nan(D.history_read(e), want) and same_nan(D.history_read(e, col0=1, n=3), want[1:])
    with pytest.raises(L.ElmkError):
        D.history_read(e, col0=2, n=3)  # cells, not columns
    with pytest.raises(L.ElmkError):
        D.gridded_history_add(0, "t_grnd", "max")  # the tape holds samples
    D.history_clear()
    D.clear_output_grid()
    assert D.lib.elmk_download_gridded(D.ctx, fid, 0, out.ctypes.data_as(C.c_void_p)) == -1
    D.set_output_grid(ptr, col, w, FILL)
    assert same_nan(D.download_gridded("t_grnd"), want)
    assert same_nan(D["t_grnd"], x)  # the state was never written
    D.close()


def test_device_bytes_account_for_the_map_and_the_accumulators():
    D = st.ELMState(3001)

    def al(b):
        return (b + 255) // 256 * 256

    b0 = D.device_bytes
    ptr, col, w = owner(D.ncols, 1000, 12)
    D.set_output_grid(ptr, col, w, FILL)
    nnz = int(ptr[-1])
    assert D.device_bytes - b0 == al(1001 * 8) + al(nnz * 4) + al(nnz * 8)
    b1 = D.device_bytes
    D.gridded_history_add(0, "t_soisno", "avg")
    D.gridded_history_add(1, "t_grnd", "max")
    cld = 1024  # 1000 cells rounded up to 64
    assert D.device_bytes - b1 == al(_levels(D, "t_soisno") * cld * 8) + al(cld * 8)
    D.history_add(0, "t_grnd", "avg")  # column entries: as before
    assert D.device_bytes - b1 == al(_levels(D, "t_soisno") * cld * 8) + al(cld * 8)
    D.history_clear()
    assert D.device_bytes == b1
    D.set_output_grid(ptr[:501], col[:ptr[500]], w[:ptr[500]], FILL)  # a smaller map replaces it
    assert D.device_bytes - b0 == al(501 * 8) + al(int(ptr[500]) * 4) + al(int(ptr[500]) * 8)
    D.clear_output_grid()
    assert D.device_bytes == b0
    D.close()
    # every counted owner at once - one full 64-column tile and a tail, 5-cell grids: the total is the sum of the layouts include/elmk.h
    # documents (the run's from elmk_run_reserve's list: series, two tables of 216-byte rows, the cursor's 256 bytes, two rings of
    # 24 doubles, a flag word and a first column per row), and every clear returns exactly its share
    n, nc, slots, msteps = 70, 5, 3, 4
    D = st.ELMState(n)
    ld, nlev, rows = D.level_stride, _levels(D, "t_soisno"), 2 * msteps
    assert ld == 128
    D.set_column_geography(np.zeros(n), np.zeros(n))  # (not counted)
    b0 = D.device_bytes
    idx = np.stack([(np.arange(n) + k) % nc for k in range(3)])  # npts 3: stored as 4 rows
    ptr, col, w = np.arange(0, n + 1, n // nc), np.arange(n), np.ones(n)
    D.set_forcing_grid(idx, np.full((3, n), 1.0 / 3.0), nc)
    D.run_reserve(slots, msteps)  # (cell records)
    D.aerosol_reserve(nc, idx[:1], np.ones((1, n)))
    D.set_output_grid(ptr, col, w, FILL)
    D.gridded_history_add(0, "t_soisno", "avg")
    D.set_shortwave_mode("coszen", 3600.0)
    D.series_record_times(0, [1.0, 1.5, 2.0])
    D.set_column_elevation(np.zeros(n), np.zeros(n))
    D.set_downscaling_groups(ptr, col, w)
    D.accum_add("t_ref2m", "runmean", 4)
    D.accum_add("t_soisno", "timeavg", 10)
    share = {"grid": al(4 * ld * 4) + al(4 * ld * 8) + al(nc * 8),
             "run": al(7 * slots * nc * 8) + al(4 * 12 * ld * 8) + al(rows * 216) + 256 + al(rows * 24 * 8) + al(rows * 4) + al(rows * 8),
             "aerosol": al(11 * 12 * nc * 8) + al(ld * 4) + al(ld * 8),
             "ogrid": al((nc + 1) * 8) + al(n * 4) + al(n * 8), "gridded": al(nlev * 64 * 8),
             "czf": ld * 8, "times": slots * 56, "topo": 2 * ld * 8,
             "groups": al((nc + 1) * 8) + al(n * 4) + al(n * 8) + al(nc * 8) + al(ld * 8),
             "accum": 16 * 21 * 48 + 256 + ld * 8 * (1 + nlev)}
    held = b0 + sum(share.values())
    assert D.device_bytes == held
    for clear, back in ((D.accum_clear, ("accum",)), (D.history_clear, ("gridded",)), (D.clear_output_grid, ("ogrid",)),
                        (D.clear_downscaling_groups, ("groups",)), (D.aerosol_clear, ("aerosol",)),
                        (D.clear_forcing_grid, ("grid", "run", "times"))):  # (the reservation and its record times go with the grid)
        clear()
        held -= sum(share[k] for k in back)
        assert D.device_bytes == held, back
    assert held == b0 + share["czf"] + share["topo"]  # nothing frees these two before the context goes
    D.close()


def test_fp32_state_library():
    """libelmk_f32.so: downloads and a gridded tape over real steps, against the aggregate of the widened fp32 values it downloads."""
    cols, scal, soil, lat, lon, rec = GR._inputs(1029, 95)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=L.F32_LIB_PATH)
    assert D.lib.elmk_state_real_bytes() == 4
    ptr, col, w = owner(D.ncols, 77, 13, shuffled=True)
    D.set_output_grid(ptr, col, w, FILL)
    entries = [(0, "t_grnd", "avg"), (0, "t_soisno", "max"), (1, "snl", "sum")]
    ids = [D.gridded_history_add(*e) for e in entries]
    ref = CellTapes(entries, np.diff(ptr) == 0)
    steps = GR.schedule(4)
    for s in range(4):
        GR.stepwise(D, rec, steps[s:s + 1], st.RUN_HISTORY)
        ref.fold({f: host_aggregate(D, f, ptr, col, w) for _, f, _ in entries})
    t = D["t_grnd"]
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))
    assert same_nan(D.download_gridded("t_grnd"), host_aggregate(D, "t_grnd", ptr, col, w))
    for k, e in enumerate(ids):
        assert same_nan(D.history_read(e), ref.result(k)), entries[k]
    D.close()


def test_gridded_output_demo(tmp_path):
    """examples/gridded_output_demo.cc: a day of 48 steps through elmk_run with a gridded AVG tape; its daily means equal the Python
    layer's run of the same tape."""
    n, nsteps, nrec = 3008, 48, 25
    cols, scal, soil, lat, lon, rec = GR._inputs(n, 97, nrec=nrec)
    steps = GR.schedule(nsteps)
    exe = build_demo("gridded_output_demo", tmp_path)
    # ownership by location on a 32 x 16 grid
    cell = RG.nearest_map(np.degrees(lat), np.degrees(lon), 32, 16)[0][0]
    ptr, col, w = RG.owner_map(cell, np.cos(lat), 32 * 16)
    extra = GR.demo_records(lat, lon, rec) + [("omap/ptr", ptr), ("omap/col", col), ("omap/w", w), ("omap/fill", np.array([FILL])), ("steps", steps)]
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, extra))
    r = run_demo(exe, tmp_path / "state.bin", tmp_path / "out.bin")
    assert "48 samples" in r.stdout and "on 512 cells" in r.stdout, r.stdout
    output = ["eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "fsa", "eflx_lwrad_out", "t_grnd", "t_soisno"]
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_output_grid(ptr, col, w, FILL)
    ids = [D.gridded_history_add(0, f, "avg") for f in output]
    D.run_reserve(nrec, nsteps)
    GR.upload_series(D, rec)
    D.run(DT, steps, st.RUN_HISTORY)
    raw = (tmp_path / "out.bin").read_bytes()
    off = 0
    for f, e in zip(output, ids):
        want = D.history_read(e)
        got = np.frombuffer(raw, np.float64, want.size, off).reshape(want.shape)
        off += want.nbytes
        assert same_nan(got, want), f
    assert off == len(raw)
    D.close()
