"""The maps and rows of the output grid's and the longwave groups' edge tests (tests/output_map_cases.py) on the host: every shape
the GPU tests name is really built - the span of exactly one tile and of one tile and a term, the cell of more than two tiles, the
workgroup without a term, the empty, one-term and all-zero-weight cells, disjoint columns where asked, few columns - and the
aggregate of edge_values on it really holds a fill, a -0.0, both kinds of NaN, an infinite and finite cells, so that a GPU
comparison on these inputs cannot pass on a case that never happened.  regrid.apply_aggregate, the reference of those tests, is
compared with a plain scalar loop at the same shapes, and the groups' norm takes its W == 0 branch.  No GPU."""
import numpy as np
import pytest

from elmkernels_amd import downscale as DSC
from elmkernels_amd import regrid as RG
from tests import output_map_cases as OM
from tests.support import same_nan

SHAPES = [(g, n) for g, cells in ((OM.AGG_CELLS, OM.OGRID_NCELLS), (OM.DS_CELLS, OM.GROUP_NCELLS)) for n in cells]
IDS = [f"wg{g}-{n}" for g, n in SHAPES]


def _map(layout, g, n, disjoint, seed=31):
    lead, mid = OM.edge_columns(n, layout)
    return OM.shape_map(n, seed, layout, cells_per_wg=g, disjoint=disjoint, lead=lead, mid=mid)


@pytest.mark.parametrize("disjoint", [False, True], ids=["repeats", "disjoint"])
@pytest.mark.parametrize("g,n", SHAPES, ids=IDS)
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_every_named_shape_is_built(layout, g, n, disjoint):
    ptr, col, w, ncols = _map(layout, g, n, disjoint)
    T = OM.AGG_TILE
    cnt = np.diff(ptr)
    span = [int(ptr[min(lo + g, n)] - ptr[lo]) for lo in range(0, n, g)]  # terms per workgroup
    assert ptr.dtype == np.int64 and col.dtype == np.int32 and w.dtype == np.float64 and ptr.size == n + 1 and ptr[0] == 0
    assert OM.MIN_NCOLS <= ncols <= OM.MAX_NCOLS and ncols <= max(int(ptr[-1]) + 3, OM.MIN_NCOLS)
    assert np.setdiff1d(np.arange(ncols), col).size >= 3  # columns in no cell
    if layout == "tiles":
        assert span[0] == T and (n <= g or span[1] == T + 1) and all(s == 3 * min(g, n - k * g) for k, s in enumerate(span) if k >= 2)
    elif layout == "big_last":
        last = min(g, n) - 1
        assert cnt[last] == 2 * T + 104 > 2 * T and span[0] > 2 * T
        assert n <= g or span[1] == 0  # the second workgroup: P0 == P1
        assert n < 2 * g or (cnt[g:2 * g].size == g and n == 2 * g + 1 and cnt[2 * g] == 3)
    elif layout == "tile_start":
        h = min(g, n) // 2
        if n > 1:  # a cell of five terms and an empty one, both exactly at the start of the first workgroup's second tile
            assert ptr[h] - ptr[0] == T and cnt[h] == 5 and cnt[h + 1] == 0 and span[0] > T
        if n > g + 3:  # a one-term cell and an empty one exactly at the start of the second workgroup's second tile
            assert ptr[g + 1] - ptr[g] == T and cnt[g + 1] == 1 and cnt[g + 2] == 0 and span[1] > T
    else:
        assert not cnt.any() and col.size == 0 and ncols == OM.MIN_NCOLS
    if layout in ("tiles", "big_last"):
        if min(g, n) > 8:
            assert cnt[0] == 0 and cnt[5] == 1
        if n >= OM.LEAD_MIN_NCELLS:
            zero = OM.special_cells(cnt)[0]
            assert zero is not None and cnt[zero] >= 2 and not w[ptr[zero]:ptr[zero + 1]].any()
            zw = (np.delete(w, np.arange(ptr[zero], ptr[zero + 1])) == 0.0).mean()
            assert 0.03 < zw < 0.10, zw  # about one weight in sixteen outside that cell
    elif layout == "tile_start" and n >= OM.LEAD_MIN_NCELLS:
        assert OM.special_cells(cnt)[0] is not None
    assert np.isfinite(w).all() and (w >= 0.0).all()
    if disjoint:
        assert np.unique(col).size == col.size
        if col.size:
            DSC.check_groups(ptr, col, w, ncols)  # what elmk_set_downscaling_groups accepts
    elif col.size:
        assert np.unique(col).size < col.size  # repeats across cells ...
        assert any(np.unique(col[ptr[c]:ptr[c + 1]]).size < cnt[c] for c in range(n))  # ... and inside one
    # the leading and the middle columns where the shape has room for them, and nowhere else
    lead, mid = OM.edge_columns(n, layout)
    _, long_, own = OM.special_cells(cnt)
    for j, c in enumerate(lead):
        at = np.nonzero(col == c)[0]
        assert at.size == 1 and at[0] == ptr[own[j]] and w[at[0]] > 0.0, (j, c)
    for j, c in enumerate(mid):
        at = np.nonzero(col == c)[0]
        cell = int(np.searchsorted(ptr, at[0], side="right")) - 1
        assert at.size == 1 and cell in long_ and ptr[cell] < at[0] < ptr[cell + 1] - 1, (j, c)
        assert (w[at[0]] == 0.0) == (j == OM.ZERO_WEIGHT_MID)


def _scalar_aggregate(ptr, col, w, x, fill):
    """The statement of include/elmk.h "output grid", one term at a time."""
    out = np.full(ptr.size - 1, float(fill))
    with np.errstate(all="ignore"):
        for i in range(ptr.size - 1):
            if ptr[i] == ptr[i + 1]:
                continue
            v = w[ptr[i]] * x[col[ptr[i]]]
            for p in range(int(ptr[i]) + 1, int(ptr[i + 1])):
                v = v + w[p] * x[col[p]]
            out[i] = v
    return out


@pytest.mark.parametrize("g,n", SHAPES, ids=IDS)
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_the_census_is_complete_and_the_reference_is_the_scalar_loop(layout, g, n):
    """edge_values on every shape: the kinds of cell census_expected names are all there, under both seeds' parities; and
    regrid.apply_aggregate equals the scalar loop bit for bit on that row, on a narrow row (every term counts in the sum's bits) and
    with fill -0.0."""
    ptr, col, w, ncols = _map(layout, g, n, disjoint=(g == OM.DS_CELLS))
    for seed in (40, 41):
        x = OM.edge_values(ncols, seed)
        seen = OM.assert_census(ptr, col, w, x, OM.FILL, n, layout, seed)
        assert sum(seen[k] for k in ("fill", "inf", "finite")) <= n
        with np.errstate(all="ignore"):
            assert same_nan(RG.apply_aggregate(ptr, col, w, x, OM.FILL), _scalar_aggregate(ptr, col, w, x, OM.FILL)), seed
        if n >= OM.LEAD_MIN_NCELLS and layout in ("tiles", "big_last") and seed % 2 == 0:
            assert all(seen[k] > 0 for k in OM.CENSUS), seen  # (every such map has an empty and a one-term cell)
    narrow = OM.edge_values(ncols, 42, span=3.0, special=False)
    got = RG.apply_aggregate(ptr, col, w, narrow, -0.0)
    assert same_nan(got, _scalar_aggregate(ptr, col, w, narrow, -0.0))
    empty = np.diff(ptr) == 0
    assert np.signbit(got[empty]).all() and np.isfinite(got).all()


def test_edge_values_order_the_samples():
    """Successive seeds give the leading columns -0.0 then +0.0, +0.0 then -0.0, +inf then -inf and the reverse, a NaN before and
    after a number; the magnitudes span 1e-300 .. 1e300 in both signs."""
    a, b = OM.edge_values(500, 6), OM.edge_values(500, 7)
    L = OM.EDGE_LEAD
    assert np.signbit(a[L[0]]) and a[L[0]] == 0.0 and not np.signbit(b[L[0]]) and b[L[0]] == 0.0
    assert not np.signbit(a[L[1]]) and a[L[1]] == 0.0 and np.signbit(b[L[1]]) and b[L[1]] == 0.0
    assert (a[L[2]], b[L[2]], a[L[3]], b[L[3]]) == (OM.INF, -OM.INF, -OM.INF, OM.INF)
    assert np.isnan(a[L[4]]) and b[L[4]] == 5e-324 and a[L[5]] == 5e-324 and np.isnan(b[L[5]]) and a[L[6]] == b[L[6]] == 1e300
    assert same_nan(a[list(OM.EDGE_MID)], OM.MID_VALUES)
    rest = np.abs(a[len(L) + len(OM.EDGE_MID):])
    assert rest.min() < 1e-250 and rest.max() > 1e250 and (a < 0).sum() > 150 and (a > 0).sum() > 150
    assert same_nan(OM.edge_values(500, 6), a)  # a function of the seed


@pytest.mark.parametrize("n", OM.GROUP_NCELLS)
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_the_groups_norm_takes_every_branch(layout, n):
    """downscale.group_norm on the group shapes: exactly 1.0 for a group without a column and for the group whose weights are all
    0.0 (W == 0), NaN for a group led by a NaN Lg, a number elsewhere; renormalise_longwave leaves every column of no group and of
    a W == 0 group its bits."""
    lead, mid = OM.edge_columns(n, layout)
    ptr, col, w, ncols = OM.shape_map(n, 33, layout, cells_per_wg=OM.DS_CELLS, disjoint=True, lead=lead[:1], mid=())
    rng = np.random.default_rng(34)
    lg, lc = rng.uniform(60.0, 590.0, ncols), rng.uniform(60.0, 590.0, ncols)
    if lead:
        lg[lead[0]] = np.nan
    norm = DSC.group_norm(lg, lc, ptr, col, w)
    cnt = np.diff(ptr)
    W = RG.apply_aggregate(ptr, col, w, np.ones(ncols), 0.0)
    zero = OM.special_cells(cnt)[0]
    assert (norm[cnt == 0] == 1.0).all() and (norm[W == 0.0] == 1.0).all()
    if zero is not None:
        assert W[zero] == 0.0 and cnt[zero] >= 2
    if lead:
        nan_group = OM.special_cells(cnt)[2][0]
        assert np.isnan(norm[nan_group]) and np.isnan(norm).sum() == 1
    live = (W > 0.0) & ~np.isnan(norm)
    assert ((norm[live] > 0.1) & (norm[live] < 10.0)).all() and (layout == "all_empty" or (norm[live] != 1.0).any())
    out = DSC.renormalise_longwave(lg, lc, ptr, col, w)
    keep = np.ones(ncols, bool)
    keep[col[np.repeat(W > 0.0, cnt)]] = False
    assert same_nan(out[keep], lc[keep]) and keep.sum() >= 3


# ---- the walk itself, restated, and slips of it that these inputs catch ------------------------------------------------------------------
def _tiled_aggregate(ptr, col, w, x, fill, cells, tile, slip=None):
    """agg_cells<cells> of k_history.hip as a host loop: a workgroup takes `cells` consecutive cells, walks their span of the map in
    tiles of `tile` products and lane t adds the products of cell c0 + t that lie in the tile.  slip: one wrong variant of it -
    "restart": the sum starts again at a tile's first product; "short_tile": a full tile is taken one product short;
    "late_first": a cell that starts exactly at a tile's start loses its first product; "zero_fill": an empty cell reads 0."""
    n = ptr.size - 1
    out = np.empty(n)
    with np.errstate(all="ignore"):
        t = w * x[col]
        for c0 in range(0, n, cells):
            c1 = min(c0 + cells, n)
            P0, P1 = int(ptr[c0]), int(ptr[c1])
            v = np.full(c1 - c0, 0.0 if slip == "zero_fill" else float(fill))
            for base in range(P0, P1, tile):
                m = min(P1 - base, tile)
                if slip == "short_tile" and m == tile:
                    m -= 1
                for k in range(c1 - c0):
                    p0, p1 = int(ptr[c0 + k]), int(ptr[c0 + k + 1])
                    lo, hi = max(p0, base), min(p1, base + m)
                    if slip == "late_first" and p0 == base and base > P0:
                        lo += 1
                    for p in range(lo, hi):
                        first = p == (lo if slip == "restart" else p0) or (slip == "late_first" and p == lo and p0 == base and base > P0)
                        v[k] = t[p] if first else v[k] + t[p]
            out[c0:c1] = v
    return out


SLIPS = {"restart": ("big_last",), "short_tile": ("tiles", "big_last", "tile_start"), "late_first": ("tile_start",),
         "zero_fill": ("tiles", "big_last", "tile_start", "all_empty")}


@pytest.mark.parametrize("g,n", [(OM.AGG_CELLS, 129), (OM.AGG_CELLS, 65), (OM.DS_CELLS, 33), (OM.DS_CELLS, 17)], ids=["wg64-129", "wg64-65", "wg16-33", "wg16-17"])
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_the_walk_restated_and_its_slips(layout, g, n):
    """The tile walk restated on the host equals regrid.apply_aggregate on every layout - the two statements the GPU tests hold the
    kernels to agree - and each one-line slip of it changes a cell of the narrow row on the layouts built to catch it: a sum that
    restarts with each tile on the cell longer than a tile, a tile taken one product short wherever a span fills a tile, a lost
    first product where a cell starts exactly at a tile's start inside a span ("tile_start": no cell of the other layouts does), a
    zero for the fill on every layout with an empty cell."""
    ptr, col, w, ncols = _map(layout, g, n, disjoint=(g == OM.DS_CELLS))
    x = OM.edge_values(ncols, 43, span=1.5, special=False)
    want = RG.apply_aggregate(ptr, col, w, x, OM.FILL)
    assert same_nan(_tiled_aggregate(ptr, col, w, x, OM.FILL, g, OM.AGG_TILE), want)
    for slip, layouts in SLIPS.items():
        got = _tiled_aggregate(ptr, col, w, x, OM.FILL, g, OM.AGG_TILE, slip)
        if layout in layouts:
            assert not same_nan(got, want), (slip, layout)
    if layout == "tile_start":  # the slip shows in exactly the cells that start at a tile's start
        late = np.nonzero(_tiled_aggregate(ptr, col, w, x, OM.FILL, g, OM.AGG_TILE, "late_first") != want)[0]
        assert set(late) <= {min(g, n) // 2, g + 1} and min(g, n) // 2 in late


def _searched_scale(lc, norm, ptr, col, cells, slip=None):
    """The second half of k_ds_lw_norm as a host loop: a workgroup of `cells` groups scales every term of its span by the norm of
    the group the term lies in, found by bisection over the span's ptr.  slip: "strict" compares sp[mid] < q (a group's first
    column goes to the group before it)."""
    out = np.array(lc, dtype=np.float64)
    n = ptr.size - 1
    for c0 in range(0, n, cells):
        ncl = min(cells, n - c0)
        sp = ptr[c0:c0 + ncl + 1]
        for q in range(int(sp[0]), int(sp[ncl])):
            lo, hi = 0, ncl
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                if (sp[mid] < q) if slip == "strict" else (sp[mid] <= q):
                    lo = mid
                else:
                    hi = mid
            out[col[q]] = out[col[q]] * norm[c0 + lo]
    return out


@pytest.mark.parametrize("n", OM.GROUP_NCELLS)
@pytest.mark.parametrize("layout", OM.LAYOUTS)
def test_the_group_search_restated_and_its_slips(layout, n):
    """The bisection restated equals downscale.renormalise_longwave on every group shape, empty groups at the front, in the middle
    and at the end of a workgroup included; a strict comparison changes a column wherever a workgroup holds two groups with
    columns."""
    ptr, col, w, ncols = OM.shape_map(n, 35, layout, cells_per_wg=OM.DS_CELLS, disjoint=True)
    rng = np.random.default_rng(36)
    lg, lc = rng.uniform(60.0, 590.0, ncols), rng.uniform(60.0, 590.0, ncols)
    norm = DSC.group_norm(lg, lc, ptr, col, w)
    want = DSC.renormalise_longwave(lg, lc, ptr, col, w)
    assert same_nan(_searched_scale(lc, norm, ptr, col, OM.DS_CELLS), want)
    if layout != "all_empty" and n > 1:
        assert not same_nan(_searched_scale(lc, norm, ptr, col, OM.DS_CELLS, "strict"), want)
