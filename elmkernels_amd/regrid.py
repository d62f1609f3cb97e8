"""Forcing on a coarser grid and output on a grid, host side (numpy only): build the per-column remap maps that
elmk_set_forcing_grid takes and the per-cell aggregation maps that elmk_set_output_grid takes, and apply both exactly as the device
does.

A map is ELL ("padded sparse rows"): idx int32 [npts, ncols] and w float64 [npts, ncols], up to npts source cells per column,
row k of every column in SoA order.  idx = -1 is padding; row 0 never holds it.  The value of column c of cell values a is

    v = w[0, c] * a[idx[0, c]];   then for k = 1 .. npts-1:  if idx[k, c] >= 0:  v = v + w[k, c] * a[idx[k, c]]

in that order, without fused multiply-adds (include/elmk.h, "forcing grid").  apply_map is that operation; the tests and a driver
that wants per-column records use it as the host reference.

Regular grids here are nlon x nlat cells of equal size in longitude and latitude, numbered cell = j * nlon + i (latitude row j
from the south, longitude column i from lon0 eastwards), cell centres at lon0 + (i + 0.5) * 360 / nlon and -90 + (j + 0.5) * 180 / nlat.
Column positions are in degrees (elmk_set_column_geography takes radians: np.radians).
"""
import numpy as np

MAX_NPTS = 8  # elmk_set_forcing_grid


def apply_map(idx, w, cells):
    """Column values of cell values `cells` ([ncells], or [nrec, ncells] for several records at once) through the map idx / w, in
    the device's operation order.  Returns float64 [ncols] (or [nrec, ncols])."""
    idx = np.asarray(idx)
    w = np.asarray(w, dtype=np.float64)
    a = np.asarray(cells, dtype=np.float64)
    if idx.ndim != 2 or idx.shape != w.shape or idx.shape[0] < 1:
        raise ValueError("idx and w must both be [npts, ncols]")
    v = w[0] * a[..., idx[0]]
    for k in range(1, idx.shape[0]):
        m = idx[k] >= 0
        t = w[k] * a[..., np.where(m, idx[k], 0)]
        v = np.where(m, v + t, v)  # padding: the sum is left as it is (no + 0.0 * a)
    return v


def _lon_index(lon, nlon, lon0):
    """Fractional longitude position in cells, [0, nlon), periodic."""
    x = np.mod((np.asarray(lon, dtype=np.float64) - lon0) / (360.0 / nlon), nlon)
    return np.where(x >= nlon, 0.0, x)  # (mod can round up to nlon)


def nearest_map(lat, lon, nlon, nlat, lon0=0.0):
    """One term of weight 1.0 per column: the cell of the regular grid that contains (lat, lon).  Longitude is periodic; latitude is
    clamped to [-90, 90] (a column on the pole takes the polar row).  Returns (idx [1, ncols] int32, w [1, ncols])."""
    lat = np.asarray(lat, dtype=np.float64)
    i = np.floor(_lon_index(lon, nlon, lon0)).astype(np.int64)
    j = np.clip(np.floor((np.clip(lat, -90.0, 90.0) + 90.0) / (180.0 / nlat)).astype(np.int64), 0, nlat - 1)
    idx = (j * nlon + np.clip(i, 0, nlon - 1)).astype(np.int32)[None, :]
    return idx, np.ones(idx.shape)


def _compact(idx, w):
    """Move the padding terms of every column behind its real ones (stable), so that row 0 holds a real term."""
    order = np.argsort(idx < 0, axis=0, kind="stable")
    return np.take_along_axis(idx, order, axis=0), np.take_along_axis(w, order, axis=0)


def bilinear_map(lat, lon, nlon, nlat, lon0=0.0, land=None):
    """Bilinear interpolation between the four cell centres around each column: four terms per column in the order (i0, j0),
    (i1, j0), (i0, j1), (i1, j1), weights (1-fx)(1-fy), fx(1-fy), (1-fx)fy, fx fy.  Longitude is periodic (a column east of the
    last centre interpolates between cells nlon-1 and 0); latitude is clamped: poleward of the outermost centres a column takes that
    row's values.  land: optional bool [ncells] (or [nlat, nlon]); corners that are not land are dropped (idx -1) and the remaining
    weights renormalised by their sum, so only land cells feed a column.  A column whose four corners are all masked (or whose
    land weights sum to 0) keeps its unmasked weights.  Returns (idx [4, ncols] int32, w [4, ncols])."""
    lat = np.asarray(lat, dtype=np.float64)
    x = _lon_index(lon, nlon, lon0) - 0.5
    i0 = np.floor(x)
    fx = x - i0
    i0 = np.mod(i0.astype(np.int64), nlon)
    i1 = np.mod(i0 + 1, nlon)
    y = np.clip((np.clip(lat, -90.0, 90.0) + 90.0) / (180.0 / nlat) - 0.5, 0.0, nlat - 1.0)
    j0 = np.minimum(np.floor(y).astype(np.int64), max(nlat - 2, 0))
    fy = y - j0
    j1 = np.minimum(j0 + 1, nlat - 1)
    idx = np.stack([j0 * nlon + i0, j0 * nlon + i1, j1 * nlon + i0, j1 * nlon + i1]).astype(np.int32)
    w = np.stack([(1.0 - fx) * (1.0 - fy), fx * (1.0 - fy), (1.0 - fx) * fy, fx * fy])
    if land is not None:
        land = np.asarray(land, dtype=bool).reshape(-1)
        if land.size != nlon * nlat:
            raise ValueError("land must have nlon * nlat cells")
        on = land[idx]
        s = np.sum(np.where(on, w, 0.0), axis=0)
        use = s > 0.0
        wm = np.where(on, w, 0.0) / np.where(use, s, 1.0)
        keep = on | ~use[None, :]
        w = np.where(use[None, :], wm, w)
        idx = np.where(keep, idx, -1).astype(np.int32)
        w = np.where(keep, w, 0.0)
        idx, w = _compact(idx, w)
    return idx, w


def from_sparse(row, col, S, ncols, ncells, one_based=False):
    """A sparse remap matrix as COO triplets - row = destination column, col = source cell, S = weight, the row / col / S variables
    of an ESMF or TempestRemap map file (one_based=True for their 1-based indices) - as an ELL map.  Each column's terms are in
    ascending source-cell order (stable for repeated cells); npts is the largest number of terms of a column, shorter columns are
    padded with idx -1, w 0.  Every column needs at least one term and at most 8.  Returns (idx [npts, ncols] int32, w)."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    if not (row.size == col.size == S.size):
        raise ValueError("row, col and S must have the same length")
    if one_based:
        row, col = row - 1, col - 1
    if row.size and (row.min() < 0 or row.max() >= ncols or col.min() < 0 or col.max() >= ncells):
        raise ValueError("row or col out of range")
    order = np.lexsort((col, row))  # by column, then by source cell (stable)
    row, col, S = row[order], col[order], S[order]
    count = np.bincount(row, minlength=ncols)
    if ncols and count.min() < 1:
        raise ValueError(f"column {int(np.argmin(count))} has no source cell")
    npts = int(count.max()) if ncols else 1
    if npts > MAX_NPTS:
        raise ValueError(f"a column has {npts} source cells, more than {MAX_NPTS}")
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    k = np.arange(row.size) - start[row]
    idx = np.full((npts, ncols), -1, np.int32)
    w = np.zeros((npts, ncols))
    idx[k, row] = col
    w[k, row] = S
    return idx, w


def slice_map(idx, w, col0, n):
    """The map of columns [col0, col0 + n) - one rank's block of decomp.block_range - with its cells renumbered: returns
    (idx_local, w_local, cells), where cells (int64, ascending) are the global cells the block reads and idx_local indexes into them.
    The rank sets ncells = cells.size and uploads records[..., cells]; apply_map(idx_local, w_local, a[cells]) is
    apply_map(idx, w, a)[col0:col0 + n] bit for bit."""
    idx = np.asarray(idx)[:, col0:col0 + n]
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64)[:, col0:col0 + n])
    cells = np.unique(idx[idx >= 0]).astype(np.int64)
    local = np.where(idx >= 0, np.searchsorted(cells, np.where(idx >= 0, idx, 0)), -1).astype(np.int32)
    return local, w, cells


# ---- output grid (elmk_set_output_grid): columns aggregated onto cells ----------------------------------------------------------
# A map is CSR by output cell: ptr int64 [ncells + 1] (ptr[0] = 0, non-decreasing), col int32 [nnz] (source columns) and w float64
# [nnz]; cell i owns terms ptr[i] .. ptr[i+1]-1.  The value of cell i of a column row x is fill for a cell without terms, else
#
#     v = w[p0] * x[col[p0]];   then for p = p0+1 .. p1-1:  v = v + w[p] * x[col[p]]
#
# in that order, without fused multiply-adds (include/elmk.h, "output grid").


def _csr(ptr, col, w):
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    col = np.asarray(col).reshape(-1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if ptr.size < 2 or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != col.size or col.size != w.size:
        raise ValueError("not a CSR map: ptr [ncells + 1] from 0, non-decreasing, ptr[-1] == len(col) == len(w)")
    return ptr, col, w


def apply_aggregate(ptr, col, w, x, fill):
    """Cell values of column values `x` ([ncols], or [nrec, ncols] for several rows at once) through the CSR map ptr / col / w, in
    the device's operation order: one rounded product per term, summed in term order from the first product.  Returns float64
    [ncells] (or [nrec, ncells]); a cell without terms is `fill`."""
    ptr, col, w = _csr(ptr, col, w)
    x = np.asarray(x, dtype=np.float64)
    ncells = ptr.size - 1
    cnt = np.diff(ptr)
    v = np.full(x.shape[:-1] + (ncells,), float(fill))
    if col.size == 0:
        return v
    t = w * x[..., col]  # every product, rounded once
    live = np.nonzero(cnt > 0)[0]
    v[..., live] = t[..., ptr[live]]
    # term k of every cell that has one, while many cells are still adding; then the few long cells one by one (add.accumulate
    # adds strictly left to right, so prepending the running value continues the same chain of roundings)
    k = 1
    while True:
        live = live[cnt[live] > k]
        if live.size <= 32:
            break
        v[..., live] = v[..., live] + t[..., ptr[live] + k]
        k += 1
    for c in live:
        seq = np.concatenate([v[..., c:c + 1], t[..., ptr[c] + k:ptr[c + 1]]], axis=-1)
        v[..., c] = np.add.accumulate(seq, axis=-1)[..., -1]
    return v


def owner_map(cell_of_col, area, ncells):
    """ELM's c2g: every column belongs to one cell (cell_of_col [ncols]; a negative entry belongs to none) and the cell value is the
    area-weighted mean of its columns, w = area_c / (sum of area over the cell's columns).  Terms are in ascending column order; a
    cell without columns has no terms.  Returns (ptr int64 [ncells + 1], col int32 [nnz], w float64 [nnz])."""
    cell = np.asarray(cell_of_col, dtype=np.int64).reshape(-1)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    if cell.size != area.size:
        raise ValueError("cell_of_col and area must both be [ncols]")
    if cell.size and cell.max() >= ncells:
        raise ValueError("cell_of_col out of range")
    cols = np.nonzero(cell >= 0)[0]
    order = cols[np.argsort(cell[cols], kind="stable")]  # by cell, ascending column inside a cell
    cnt = np.bincount(cell[cols], minlength=ncells)
    tot = np.bincount(cell[cols], weights=area[cols], minlength=ncells)
    if np.any((cnt > 0) & ~(tot > 0.0)) or not np.all(np.isfinite(tot)):
        raise ValueError("a cell's columns must have a finite, positive total area")
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return ptr, order.astype(np.int32), area[order] / tot[cell[order]]


def from_sparse_cells(row, col, S, ncells, ncols, one_based=False):
    """A land -> atmosphere map file's triplets - row = destination cell, col = source column, S = weight (the row / col / S variables
    of an ESMF or TempestRemap file; one_based=True for their 1-based indices) - as a CSR map by cell.  Each cell's terms are in
    ascending column order, stable for a repeated column; a cell without triplets has no terms.  Returns (ptr, col, w)."""
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    S = np.asarray(S, dtype=np.float64).reshape(-1)
    if not (row.size == col.size == S.size):
        raise ValueError("row, col and S must have the same length")
    if one_based:
        row, col = row - 1, col - 1
    if row.size and (row.min() < 0 or row.max() >= ncells or col.min() < 0 or col.max() >= ncols):
        raise ValueError("row or col out of range")
    order = np.lexsort((col, row))  # by cell, then by column (stable)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=ncells))]).astype(np.int64)
    return ptr, col[order].astype(np.int32), S[order]


def slice_output_map(ptr, col, w, col0, n):
    """One rank's part of an output map when it holds columns [col0, col0 + n) (decomp.block_range).  Returns (ptr_l, col_l, w_l,
    cells, straddling): the local map of the cells whose every term lies in the block, with columns renumbered from col0; `cells`
    (int64, ascending) their global ids, so apply_aggregate(ptr_l, col_l, w_l, x[col0:col0 + n], fill) is
    apply_aggregate(ptr, col, w, x, fill)[cells] bit for bit; and `straddling` (int64, ascending) the cells with terms both inside
    and outside the block.  Cells without terms are in no rank's list (they are fill everywhere).  Combining a straddling cell across
    ranks is left to the driver."""
    ptr, col, w = _csr(ptr, col, w)
    ncells = ptr.size - 1
    cell_of_term = np.repeat(np.arange(ncells), np.diff(ptr))
    inside = (col >= col0) & (col < col0 + n)
    nin = np.bincount(cell_of_term, weights=inside, minlength=ncells).astype(np.int64)
    cnt = np.diff(ptr)
    cells = np.nonzero((cnt > 0) & (nin == cnt))[0].astype(np.int64)
    straddling = np.nonzero((nin > 0) & (nin < cnt))[0].astype(np.int64)
    take = np.isin(cell_of_term, cells)
    ptr_l = np.concatenate([[0], np.cumsum(cnt[cells])]).astype(np.int64)
    return ptr_l, (col[take] - col0).astype(np.int32), w[take].copy(), cells, straddling
