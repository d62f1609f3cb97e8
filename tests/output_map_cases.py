"""The inputs of the output grid's and the longwave groups' edge tests, host and device (include/elmk.h "output grid", "downscaling"):
CSR maps at the shapes the shared tile walk of k_history.hip (agg_cells<CELLS>: k_ogrid_aggregate and k_hist_accumulate_cells with 64
cells per workgroup, k_ds_lw_norm with 16, LDS tiles of 2048 terms) can go wrong at, a wide-range column row with every edge value
at a known place of such a map, the census that shows which kinds of cell an aggregate held, and the two host references the
gridded tests share (the aggregate of a download, the fold of the per-step aggregates).  tests/irrigation_supply_cases.py: shape_map
is the same builder for k_irrigation_supply's own walk (tiles of 1024 terms, every column in at most one cell)."""
import numpy as np

from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests.run_cases import NumpyTapes

NAN, INF = float("nan"), float("inf")
FILL = 1.0e36  # ELM's spval
AGG_CELLS, DS_CELLS, AGG_TILE = 64, 16, 2048  # k_history.hip: cells per workgroup of the output grid and of the groups, terms per LDS tile
LAYOUTS = ("tiles", "big_last", "tile_start", "all_empty")
OGRID_NCELLS = (1, 63, 64, 65, 129)  # a workgroup of 64 cells: one cell, a workgroup less one, one, one and a cell, two and a cell
GROUP_NCELLS = (1, 15, 16, 17, 33)  # the same around a workgroup of 16 groups
MAX_NCOLS = 9000

# The edge values and their columns.  EDGE_LEAD[j] leads a cell of its own (shape_map's `lead`) and holds LEAD_VALUES[j] in a row
# of even seed and LEAD_VALUES[j ^ 1] in one of odd seed (the last keeps its value): samples seed, seed + 1, ... of one column are
# -0.0 then +0.0, +0.0 then -0.0, +inf then -inf, ... .  EDGE_MID[j] sits in the middle of long cell j // 2 (shape_map's `mid`): +inf and
# -inf with positive weights in one cell (inf + -inf), +inf with weight 0.0 in the next (0.0 * inf), then 1e300 twice, -0.0 and 5e-324.
LEAD_VALUES = (-0.0, 0.0, INF, -INF, NAN, 5e-324, 1e300)
MID_VALUES = (INF, -INF, INF, 1e300, 1e300, 1e300, -0.0, 5e-324)
EDGE_LEAD = tuple(range(len(LEAD_VALUES)))
EDGE_MID = tuple(range(len(LEAD_VALUES), len(LEAD_VALUES) + len(MID_VALUES)))
ZERO_WEIGHT_MID = 2  # the term of mid[2] has weight exactly 0.0
MIN_NCOLS = 70  # every map spans at least this many columns, so that the edge columns exist
LEAD_MIN_NCELLS = 15  # from this many cells on a "tiles" or "big_last" map has cells enough for every leading column
CENSUS = ("fill", "neg_zero", "nan_zero_times_inf", "nan_inf_minus_inf", "inf", "finite")


def edge_columns(ncells, layout):
    """(lead, mid) for shape_map at this shape: none on a map without a term, the middle columns alone below LEAD_MIN_NCELLS cells."""
    if layout == "all_empty":
        return (), ()
    return (EDGE_LEAD if ncells >= LEAD_MIN_NCELLS else ()), EDGE_MID


def cell_counts(ncells, seed, layout, cells_per_wg, tile=AGG_TILE):
    """Terms per cell of shape_map (the first draws of its generator).  Returns (cnt int64 [ncells], rng)."""
    assert layout in LAYOUTS and ncells >= 1
    rng = np.random.default_rng(seed)
    cnt = np.zeros(ncells, np.int64)
    G = cells_per_wg

    def deal(lo, hi, total):
        """Cells lo .. hi - 1 share `total` terms: the first none and the sixth one where the group has more than eight cells, the rest two or more."""
        m = hi - lo
        if m == 1:
            cnt[lo] = total
            return
        fixed = {lo: 0, lo + 5: 1} if m > 8 else {}
        for c, v in fixed.items():
            cnt[c] = v
        rest = np.array([c for c in range(lo, hi) if c not in fixed])
        left = total - sum(fixed.values())
        assert left >= 2 * rest.size
        cnt[rest] = 2 + rng.multinomial(left - 2 * rest.size, np.full(rest.size, 1.0 / rest.size))

    g0 = min(G, ncells)
    if layout == "tiles":
        deal(0, g0, tile)
        if ncells > G:
            deal(G, min(2 * G, ncells), tile + 1)
        cnt[2 * G:] = 3
    elif layout == "big_last":
        if g0 > 1:
            deal(0, g0 - 1, 4 * (g0 - 1))
        cnt[g0 - 1] = 2 * tile + 104
        cnt[2 * G:] = 3
    elif layout == "tile_start":
        if g0 < 4:
            cnt[0] = tile
        else:
            h = g0 // 2
            deal(0, h, tile)
            cnt[h], cnt[h + 1], cnt[h + 2:g0] = 5, 0, 3
        if ncells > G + 3:
            cnt[G], cnt[G + 1], cnt[G + 2], cnt[G + 3:2 * G] = tile, 1, 0, 3
        else:
            cnt[G:] = 3
        cnt[2 * G:] = 3
    return cnt, rng


def special_cells(cnt, tile=AGG_TILE):
    """The cells shape_map treats specially, from the counts alone: (zero, long, own).  zero: the cell of two or more terms whose
    weights are all 0.0 - the second cell of 2 .. tile / 2 terms where there are three such cells, else None.  long: up to four cells
    of six or more terms, longest first, that take the `mid` columns.  own: the cells that take the `lead` columns, in order - the
    cells of one term, then those of two or more - without zero and long."""
    mod = [int(c) for c in np.nonzero((cnt >= 2) & (cnt <= tile // 2))[0]]
    zero = mod[1] if len(mod) >= 3 else None
    by_len = [int(c) for c in np.argsort(-cnt, kind="stable") if cnt[c] >= 6 and c != zero]
    long_ = by_len[:4]
    own = [int(c) for c in np.nonzero(cnt == 1)[0]] + [int(c) for c in np.nonzero(cnt >= 2)[0] if c != zero and c not in long_]
    return zero, long_, own


def shape_map(ncells, seed, layout="tiles", cells_per_wg=AGG_CELLS, tile=AGG_TILE, disjoint=False, lead=(), mid=()):
    """A CSR map at the shapes a walk in tiles of `tile` terms by workgroups of `cells_per_wg` consecutive cells can go wrong at, over
    just enough columns (three more lie in no cell; never fewer than MIN_NCOLS columns in all).
      "tiles":     the first workgroup's terms number exactly `tile`, the second's (where there is one) exactly `tile + 1`, the
                   cells behind the second workgroup hold three terms each; where a workgroup has more than eight cells its first
                   cell is empty and its sixth holds one term.
      "big_last":  the last cell of the first workgroup holds 2 * tile + 104 terms, more than two tiles; every cell of the second
                   workgroup is empty, so that its span is empty (P0 == P1); the cell behind it holds three terms.
      "tile_start": cells that start exactly where a tile starts inside a span: the first half of the first workgroup's cells
                   hold exactly `tile` terms, the next cell holds five, the one behind it none; the second workgroup (where it has
                   more than three cells) begins with a cell of exactly `tile` terms, a cell of one term and an empty cell; every
                   other cell holds three terms.
      "all_empty": no cell has a term.
    disjoint=True: every column in at most one cell (the longwave groups require it).  False: the other columns are drawn with
    repeats, across and inside cells, as in a sparse map file.
    Weights are finite and >= 0, about one in sixteen exactly 0.0, and one cell of two or more terms has all weights 0.0
    (special_cells: zero; none on a map of fewer than three moderate cells).  The layouts are those of irrigation_supply_cases.shape_map
    and "tile_start", which that walk's tests have no like of.
    lead: columns that become the first term of a cell of their own each, with a positive weight (special_cells: own, in order: the
    one-term cells first).  mid: columns that become terms in the middle of the longest cells, two to a cell (special_cells: long),
    with positive weights but for mid[ZERO_WEIGHT_MID], whose weight is 0.0.  Neither kind of column occurs anywhere else.
    The last term of a full tile of a workgroup's span and the term behind it have positive weights (outside the all-zero cell),
    so that a walk that loses either shows in the sum.
    Returns (ptr int64, col int32, w float64, ncols)."""
    cnt, rng = cell_counts(ncells, seed, layout, cells_per_wg, tile)
    G = cells_per_wg
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nnz = int(ptr[-1])
    lead, mid = [int(i) for i in lead], [int(i) for i in mid]
    placed = lead + mid
    ncols = max(nnz + 3, MIN_NCOLS) if disjoint else max(nnz // 2 + 3 + len(EDGE_LEAD) + len(EDGE_MID), MIN_NCOLS)
    assert len(set(placed)) == len(placed) and all(0 <= i < ncols for i in placed)
    zero, long_, own = special_cells(cnt, tile)
    assert len(own) >= len(lead), "too few cells for the leading columns"
    assert not mid or long_, "no long cell for the middle columns"
    col = np.full(nnz, -1, np.int64)
    lead_at = [int(ptr[c]) for c in own[:len(lead)]]
    mid_at = []
    for j in range(len(mid)):
        c = long_[(j // 2) % len(long_)]
        at = int(ptr[c]) + int(cnt[c]) // 2 + j % 2 + 2 * (j // 2 // len(long_))
        assert ptr[c] < at < ptr[c + 1] - 1, "the long cell is too short for its middle columns"
        mid_at.append(at)
    col[lead_at] = lead
    col[mid_at] = mid
    others = rng.permutation(np.setdiff1d(np.arange(ncols), placed))
    pool = others[:-3]  # (the last three of the permutation lie in no cell)
    todo = np.nonzero(col < 0)[0]
    if disjoint:
        assert pool.size >= todo.size
        col[todo] = pool[:todo.size]
    elif todo.size:
        col[todo] = rng.choice(pool, todo.size)
        twice = [c for c in np.nonzero(cnt >= 2)[0] if c not in own[:len(lead)] and ptr[c] + 1 not in mid_at]
        col[ptr[twice[0]] + 1] = col[ptr[twice[0]]]  # a column twice in one cell
    w = rng.uniform(0.05, 1.5, nnz) / np.repeat(np.maximum(cnt, 1), cnt)
    w[rng.random(nnz) < 1.0 / 16.0] = 0.0
    edge_at = [p for lo in range(0, ncells, G) for b in range(int(ptr[lo]) + tile, int(ptr[min(lo + G, ncells)]) + 1, tile)
               for p in (b - 1, b) if p < ptr[min(lo + G, ncells)]]  # the terms on either side of a tile's end inside a span
    for at in lead_at + mid_at + edge_at:
        w[at] = w[at] if w[at] > 0.0 else 0.25
    if len(mid) > ZERO_WEIGHT_MID:
        w[mid_at[ZERO_WEIGHT_MID]] = 0.0
    if zero is not None:
        w[ptr[zero]:ptr[zero + 1]] = 0.0
    # the shape, as stated
    g0 = min(G, ncells)
    assert (np.diff(ptr) == cnt).all() and col.min(initial=0) >= 0 and col.max(initial=0) < ncols
    assert np.isfinite(w).all() and (w >= 0.0).all()
    assert ncols <= MAX_NCOLS and np.setdiff1d(np.arange(ncols), col).size >= 3
    if layout == "tiles":
        assert ptr[g0] - ptr[0] == tile and (ncells <= G or ptr[min(2 * G, ncells)] - ptr[G] == tile + 1) and (cnt[2 * G:] == 3).all()
    elif layout == "big_last":
        assert cnt[g0 - 1] == 2 * tile + 104 and not cnt[G:2 * G].any() and (cnt[2 * G:] == 3).all()
    elif layout == "tile_start":
        h = g0 // 2
        assert g0 < 4 or (ptr[h] - ptr[0] == tile and cnt[h] == 5 and cnt[h + 1] == 0)
        assert ncells <= G + 3 or (ptr[G + 1] - ptr[G] == tile and cnt[G + 1] == 1 and cnt[G + 2] == 0)
    else:
        assert nnz == 0
    for lo in range(0, min(2 * G, ncells), G):
        if min(lo + G, ncells) - lo > 8 and (layout == "tiles" or (layout == "big_last" and lo == 0)):
            assert cnt[lo] == 0 and cnt[lo + 5] == 1
    if disjoint:
        assert np.unique(col).size == nnz
    if zero is not None:
        assert cnt[zero] >= 2 and not w[ptr[zero]:ptr[zero + 1]].any()
    return ptr, col.astype(np.int32), w, ncols


def edge_values(ncols, seed, span=300.0, special=True):
    """A wide-range fp64 row: magnitudes log-uniform in 10^-span .. 10^span, of both signs; with special, LEAD_VALUES in the columns
    EDGE_LEAD (paired values swapped in a row of odd seed) and MID_VALUES in the columns EDGE_MID."""
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-span, span, ncols) * rng.choice([-1.0, 1.0], ncols)
    if special:
        assert ncols >= MIN_NCOLS
        for j, c in enumerate(EDGE_LEAD):
            x[c] = LEAD_VALUES[j ^ 1 if seed % 2 and j < 6 else j]  # pairs (0, 1), (2, 3), (4, 5); the seventh stays
        x[list(EDGE_MID)] = MID_VALUES
    return x


def census(ptr, col, w, x, fill):
    """Which kinds of cell the aggregate of row x holds: name -> count.  fill: a cell without a term; neg_zero: a cell of one -0.0
    term with a positive weight, which reads -0.0; nan_zero_times_inf: a NaN cell with a product 0.0 * inf; nan_inf_minus_inf: a NaN
    cell that adds a +inf and a -inf product; inf: an infinite cell; finite: a finite cell with terms."""
    ptr, w, x = np.asarray(ptr), np.asarray(w, dtype=np.float64), np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = RG.apply_aggregate(ptr, col, w, x, fill)
    cnt = np.diff(ptr)
    ncells = cnt.size
    cell = np.repeat(np.arange(ncells), cnt)
    xv = x[col]
    with np.errstate(all="ignore"):
        t = w * xv
    has = lambda m: np.bincount(cell[m], minlength=ncells) > 0  # noqa: E731
    first = np.minimum(ptr[:-1], max(w.size - 1, 0))
    one_pos = (cnt == 1) & ((w[first] > 0.0) if w.size else False)
    return {"fill": int((cnt == 0).sum()), "neg_zero": int((one_pos & (g == 0.0) & np.signbit(g)).sum()),
            "nan_zero_times_inf": int((np.isnan(g) & has((w == 0.0) & np.isinf(xv))).sum()),
            "nan_inf_minus_inf": int((np.isnan(g) & has(t == INF) & has(t == -INF)).sum()),
            "inf": int(np.isinf(g).sum()), "finite": int((np.isfinite(g) & (cnt > 0)).sum())}


def census_expected(ncells, layout, cnt, seed=0):
    """The kinds census must count at least once on a map of this shape whose columns hold edge_values(ncols, seed) (edge_columns
    placed).  The -0.0 leads the first one-term cell in a row of even seed and the second, where there is one, in a row of odd seed."""
    if layout == "all_empty":
        return ("fill",)
    want = ["nan_zero_times_inf", "nan_inf_minus_inf"]  # the middle columns: every shape with a term has a long cell
    if (cnt == 0).any():
        want.append("fill")
    if ncells >= LEAD_MIN_NCELLS:
        want += ["inf", "finite"] + (["neg_zero"] if (cnt == 1).sum() > seed % 2 else [])
    return tuple(want)


def assert_census(ptr, col, w, x, fill, ncells, layout, seed=0):
    """census, and that it holds every kind census_expected names: a comparison on this row checked those cells."""
    seen = census(ptr, col, w, x, fill)
    missing = [k for k in census_expected(ncells, layout, np.diff(ptr), seed) if not seen[k]]
    assert not missing, (ncells, layout, missing, seen)
    return seen


# ---- the host references of the gridded tests ------------------------------------------------------------------------------------------
def host_aggregate(D, name, ptr, col, w, fill=FILL):
    """The reference: the field downloaded, widened to fp64, every level aggregated on the host.  [ncells] or [ncells, nlev]."""
    x = D.download(name, layout=st.LAYOUT_SOA).astype(np.float64)
    with np.errstate(all="ignore"):  # (edge rows: 0.0 * inf, inf + -inf)
        g = RG.apply_aggregate(ptr, col, w, x, fill)
    return g if g.ndim == 1 else np.ascontiguousarray(g.T)


class CellTapes(NumpyTapes):
    """The host fold of the per-step aggregates; a cell without terms reads fill under every op."""

    def __init__(self, entries, empty, fill=FILL):
        super().__init__(entries)
        self.empty = empty
        self.fill = fill

    def result(self, k):
        r = super().result(k)
        return np.where(self.empty if r.ndim == 1 else self.empty[:, None], self.fill, r)
