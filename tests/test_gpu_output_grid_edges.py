"""The output grid at the edges of its tile walk (k_history.hip: agg_cells<64> under k_ogrid_aggregate and k_hist_accumulate_cells):
maps whose workgroup spans are exactly one LDS tile and one tile and a term, a cell of more than two tiles, a workgroup without a
term, cells that start exactly at a tile's start and a map without a term (tests/output_map_cases.py: shape_map), at 1, 63, 64, 65 and 129 cells, under a wide-range row with
NaN, +-inf, signed zeros, a subnormal and 1e300 at known places (edge_values) and narrow rows in which every term shows in the
sum's bits; every stored type; fill 1e36 and -0.0; gridded tapes under all five ops with a reset of one tape in the middle; and the
three ways the one launch's two block counts can differ.  Everything is bit for bit against regrid.apply_aggregate of the same
context's downloads and the host folds (a NaN matches a NaN), in both builds; the census of each row is asserted next to the
comparison that used it (tests/test_output_map_cases_host.py shows on the CPU that it can be met).  No physics step runs."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from tests import output_map_cases as OM
from tests.run_cases import NumpyTapes
from tests.support import same, same_nan

pytestmark = pytest.mark.gpu

FILL = OM.FILL
OPS = ("avg", "sum", "max", "min", "inst")
F64, F32 = None, L.F32_LIB_PATH


def _id(v):
    return "f32" if v == F32 else "f64" if v is None else None


def _cases(f32_at):
    """(layout, ncells, library): the fp64 build at every shape, libelmk_f32.so at the shapes of f32_at."""
    out = [(layout, n, F64) for layout in OM.LAYOUTS for n in OM.OGRID_NCELLS]
    return out + [(layout, n, F32) for layout, n in f32_at]


def _map(layout, ncells, seed):
    lead, mid = OM.edge_columns(ncells, layout)
    return OM.shape_map(ncells, seed, layout, cells_per_wg=OM.AGG_CELLS, disjoint=False, lead=lead, mid=mid)


def _rows(D, seed, f32):
    """One sample of every source, uploaded directly: t_grnd the wide-range row with the edge values (in the fp32 build the range
    fp32 holds, rounded to fp32 on the host: 1e300 is +inf there and 5e-324 is 0), every level of t_soisno a narrow row of its own
    (three decades, both signs: every term of a cell shows in the sum's bits), snl over 0 .. 5 (elmk_upload refuses any other: snl
    indexes the level arrays), altmax_indx - the I32 field that takes any value - over the whole of I32 with INT32_MIN among the
    negatives, veg_active over the whole of U8, err_flags over the whole of U32."""
    n = D.ncols
    rng = np.random.default_rng(seed + 1000)
    t = OM.edge_values(n, seed, span=30.0 if f32 else 300.0)
    soi = np.stack([OM.edge_values(n, 100 * seed + lev + 1, span=1.5, special=False) for lev in range(D.fields["t_soisno"][1])], axis=1)
    if f32:
        with np.errstate(over="ignore"):
            t, soi = t.astype(np.float32).astype(np.float64), soi.astype(np.float32).astype(np.float64)
    D["t_grnd"] = t
    D["t_soisno"] = soi
    D["snl"] = rng.integers(0, 6, n).astype(np.int32)
    idx = rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)
    idx[::5] = -np.abs(idx[::5])
    idx[n // 2] = -(1 << 31)
    D["altmax_indx"] = idx
    D["veg_active"] = rng.integers(0, 256, n).astype(np.uint8)
    flags = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    flags[::7] |= np.uint32(1 << 31)
    D["err_flags"] = flags
    assert same_nan(D["t_grnd"], t) and same(D["err_flags"], flags) and (D["err_flags"] >= (1 << 31)).any() and same(D["altmax_indx"], idx)


# ---- a. downloads -------------------------------------------------------------------------------------------------------------------------
SOURCES = (("t_grnd", (0,)), ("t_soisno", (0, 19)), ("snl", (0,)), ("altmax_indx", (0,)), ("veg_active", (0,)), ("err_flags", (0,)))


@pytest.mark.parametrize("layout,ncells,lib_path", _cases([("tiles", 129), ("big_last", 65), ("tile_start", 129)]), ids=_id)
def test_download_gridded_on_every_map_shape(layout, ncells, lib_path):
    """elmk_download_gridded of every stored type against the host aggregate of the same context's download; at "big_last" / 129
    once more with fill -0.0.  A cell without a term has the fill's bits."""
    ptr, col, w, ncols = _map(layout, ncells, 81)
    D = st.ELMState(ncols, lib_path=lib_path)
    assert D.lib.elmk_state_real_bytes() == (4 if lib_path else 8)
    _rows(D, 82, lib_path is not None)
    empty = np.diff(ptr) == 0
    for fill in (FILL, -0.0) if (layout, ncells) == ("big_last", 129) else (FILL,):
        D.set_output_grid(ptr, col, w, fill)
        seen = OM.assert_census(ptr, col, w, D["t_grnd"], fill, ncells, layout, seed=82)
        print(f"{layout}/{ncells} fill={fill!r} census: {seen}")
        for name, levels in SOURCES:
            want = OM.host_aggregate(D, name, ptr, col, w, fill)
            for lev in levels:
                got = D.download_gridded(name, level=lev)
                ref = want if want.ndim == 1 else want[:, lev]
                bad = np.nonzero(~((got.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(got) & np.isnan(ref))))[0]
                assert not bad.size, (layout, ncells, fill, name, lev, bad[:5].tolist(), got[bad[:5]].tolist(), ref[bad[:5]].tolist())
                assert same(got[empty], np.full(int(empty.sum()), fill))
            if name != "t_grnd" and layout != "all_empty":
                assert np.isfinite(want).all() and np.unique(want[~empty]).size > (~empty).sum() // 2  # (narrow rows: sums that tell)
    D.close()


# ---- b. gridded tapes at the map shapes ------------------------------------------------------------------------------------------------------
TAPE_FIELDS = ("t_grnd", "t_soisno", "snl")
GRIDDED = [(k % 2, f, op) for k, (f, op) in enumerate((f, op) for f in TAPE_FIELDS for op in OPS)]  # both tapes hold every field
COLUMN = [(0, "t_grnd", "sum"), (1, "snl", "max")]
C0, M = 61, 7  # a partial read across the boundary between the first two workgroups (cells 61 .. 67)


def _check(D, ids, ref, what, part=None):
    for k, e in enumerate(ids):
        want = ref.result(k)
        assert same_nan(D.history_read(e), want), (what, ref.entries[k])
        if part:
            c0, m = part
            assert same_nan(D.history_read(e, col0=c0, n=m), want[c0:c0 + m]), (what, ref.entries[k], "part")
            if want.ndim == 2:
                assert same_nan(D.history_read(e, col0=c0, n=m, layout=st.LAYOUT_SOA), want[c0:c0 + m].T), (what, ref.entries[k], "part, SoA")


@pytest.mark.parametrize("lib_path", [F64, F32], ids=_id)
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_gridded_tapes_on_the_map_shapes(layout, lib_path):
    """129 cells; all five ops on t_grnd, the 20 levels of t_soisno and snl as gridded entries over two tapes, two column entries;
    four accumulates with the fields overwritten in between - sample k of t_grnd is edge_values(seed + k), so that the cell a +inf
    leads reads -inf in the next sample and the one-term cells read -0.0 then +0.0 and the reverse - and tape 0 reset after the
    second while tape 1 keeps going: the counts are [2, 4].  Against the host fold of the per-sample aggregates, whole and for cells
    61 .. 67."""
    ncells, seed = 129, 90
    f32 = lib_path is not None
    ptr, col, w, ncols = _map(layout, ncells, 83)
    D = st.ELMState(ncols, lib_path=lib_path)
    D.set_output_grid(ptr, col, w, FILL)
    gid = [D.gridded_history_add(*e) for e in GRIDDED]
    cid = [D.history_add(*e) for e in COLUMN]
    ref, cref = OM.CellTapes(GRIDDED, np.diff(ptr) == 0), NumpyTapes(COLUMN)
    for k in range(4):
        _rows(D, seed + k, f32)
        OM.assert_census(ptr, col, w, D["t_grnd"], FILL, ncells, layout, seed=seed + k)
        D.history_accumulate()
        with np.errstate(invalid="ignore"):  # (inf + -inf is one of the cases)
            ref.fold({f: OM.host_aggregate(D, f, ptr, col, w) for f in TAPE_FIELDS})
            cref.fold({f: D[f] for _, f, _ in COLUMN})
        if k == 1:
            D.history_reset(0)
            ref.reset(0)
            cref.reset(0)
    assert [D.history_count(t) for t in (0, 1)] == ref.count[:2] == [2, 4]
    _check(D, gid, ref, layout, part=(C0, M))
    _check(D, cid, cref, layout)
    if layout != "all_empty":  # by value, the cases the samples were ordered for
        _, _, own = OM.special_cells(np.diff(ptr))
        read = {(f, op): D.history_read(e) for e, (_, f, op) in zip(gid, GRIDDED)}
        assert np.isnan(read["t_grnd", "sum"][own[2]]) and np.isnan(read["t_grnd", "sum"][own[3]])  # +inf then -inf, and the reverse
        for op in ("max", "min"):  # -0.0 then +0.0: the first one stays
            z = read["t_grnd", op][own[0]]
            assert z == 0.0 and np.signbit(z), (op, z)
        assert np.diff(ptr)[own[0]] == 1
        if layout != "big_last":  # (a second one-term cell: +0.0 then -0.0)
            assert np.diff(ptr)[own[1]] == 1
            for op in ("max", "min"):
                z = read["t_grnd", op][own[1]]
                assert z == 0.0 and not np.signbit(z), (op, z)
        assert np.isnan(read["t_grnd", "max"][own[4]]) and np.isnan(read["t_grnd", "min"][own[4]])  # a NaN sticks
    D.close()


# ---- c. the launch's two block counts --------------------------------------------------------------------------------------------------------
def _block_count_context(ncols, ptr, col, w, gridded, column, with_grid=True):
    """Three accumulates of directly uploaded rows; returns the results of the gridded and of the column entries after checking
    them against the host folds."""
    D = st.ELMState(ncols)
    ids = {}
    if with_grid:
        D.set_output_grid(ptr, col, w, FILL)
    # registered in turn: the two kinds of entry share one table of ids
    order = [("g", e) for e in (gridded if with_grid else [])] + [("c", e) for e in column]
    order = order[::2] + order[1::2]
    for kind, e in order:
        ids[kind, e] = D.gridded_history_add(*e) if kind == "g" else D.history_add(*e)
    gref, cref = OM.CellTapes(gridded, np.diff(ptr) == 0), NumpyTapes(column)
    fields = sorted({f for _, f, _ in gridded + column})
    for k in range(3):
        _rows(D, 95 + k, False)
        D.history_accumulate()
        with np.errstate(invalid="ignore"):
            if with_grid and gridded:
                gref.fold({f: OM.host_aggregate(D, f, ptr, col, w) for f in fields})
            if column:
                cref.fold({f: D[f] for f in fields})
    got_g = [D.history_read(ids["g", e]) for e in gridded] if with_grid else []
    got_c = [D.history_read(ids["c", e]) for e in column]
    for k, g in enumerate(got_g):
        assert same_nan(g, gref.result(k)), (ncols, gridded[k])
    for k, c in enumerate(got_c):
        assert same_nan(c, cref.result(k)), (ncols, column[k])
    tapes = {t for t, _, _ in (gridded if with_grid else []) + column}
    assert all(D.history_count(t) == 3 for t in tapes)
    D.close()
    return got_g, got_c


def test_more_cell_blocks_than_pair_blocks():
    """70 columns (one block of column pairs) under a 129-cell map (three blocks of cells): two column entries and three gridded
    ones in one launch; then gridded entries alone (no column row: the launch is sized by the cells); the column entries have the
    bits of a context without an output grid."""
    ncols = 70
    ptr, col, w, _ = _map("tiles", 129, 84)
    col = (col % (ncols - 3)).astype(np.int32)  # the same shape over 67 columns; three lie in no cell
    gridded = [(0, "t_grnd", "sum"), (1, "t_soisno", "max"), (2, "snl", "avg")]
    column = [(0, "t_grnd", "avg"), (1, "snl", "min")]
    got_g, got_c = _block_count_context(ncols, ptr, col, w, gridded, column)
    only_g, none = _block_count_context(ncols, ptr, col, w, gridded, [])
    assert not none and all(same_nan(a, b) for a, b in zip(only_g, got_g))
    _, plain = _block_count_context(ncols, ptr, col, w, gridded, column, with_grid=False)
    assert len(plain) == len(got_c) and all(same(a, b) for a, b in zip(plain, got_c))  # the very bits, a NaN's included
    assert np.isfinite(got_g[1]).all() and np.isfinite(got_g[2][np.diff(ptr) > 0]).all()


def test_more_pair_blocks_than_cell_blocks():
    """1100 columns (three blocks of column pairs) under a map of one cell (one block of cells, a span of exactly one tile): the
    cell row's workgroups past the first leave at once; the column entries have the bits of a context without an output grid."""
    ncols = 1100
    ptr, col, w, _ = _map("tiles", 1, 85)
    col = (col % (ncols - 3)).astype(np.int32)
    gridded = [(0, "t_soisno", "avg")]
    column = [(0, "t_grnd", "max"), (1, "t_soisno", "sum")]
    got_g, got_c = _block_count_context(ncols, ptr, col, w, gridded, column)
    _, plain = _block_count_context(ncols, ptr, col, w, gridded, column, with_grid=False)
    assert len(plain) == len(got_c) and all(same(a, b) for a, b in zip(plain, got_c))  # the very bits, a NaN's included
    assert got_g[0].shape == (1, 20) and np.isfinite(got_g[0]).all() and ptr[1] == OM.AGG_TILE
