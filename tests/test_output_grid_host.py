"""Output on a grid without a GPU: the C ABI of include/elmk.h ("output grid") declared, in the ctypes table and exported by both builds,
and the host side of elmkernels_amd/regrid.py - apply_aggregate in the device's operation order, owner_map, from_sparse_cells and
slice_output_map."""
import os
import re

import numpy as np

from elmkernels_amd import _lib as L
from elmkernels_amd import decomp
from elmkernels_amd import regrid as R
from tests.support import ROOT, same_nan

HEADER = open(os.path.join(ROOT, "include", "elmk.h")).read()
ENTRY_POINTS = {"elmk_set_output_grid", "elmk_clear_output_grid", "elmk_download_gridded", "elmk_gridded_history_add"}


def loop_aggregate(ptr, col, w, x, fill):
    """include/elmk.h's rule, one Python float operation at a time."""
    out = []
    for i in range(len(ptr) - 1):
        p0, p1 = int(ptr[i]), int(ptr[i + 1])
        if p0 == p1:
            out.append(float(fill))
            continue
        v = float(w[p0]) * float(x[col[p0]])
        for p in range(p0 + 1, p1):
            v = v + float(w[p]) * float(x[col[p]])
        out.append(v)
    return np.array(out, dtype=np.float64)


def _ownership(ncols, ncells, seed, unowned=0.1):
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, ncells, ncols)
    cell[rng.random(ncols) < unowned] = -1
    area = rng.random(ncols) * 3.0 + 0.01
    return cell, area


def test_output_grid_entry_points_are_declared_and_exported():
    declared = set(re.findall(r"^int (elmk_\w+)\(", HEADER, re.M))
    assert ENTRY_POINTS <= declared
    assert ENTRY_POINTS <= set(L.SIGNATURES)
    for path in (L.LIB_PATH, L.F32_LIB_PATH):
        lib = L.load(path)  # declares every symbol of the table; raises if one is missing
        for name in ENTRY_POINTS:
            assert getattr(lib, name) is not None


def test_apply_aggregate_equals_a_plain_loop_bit_for_bit():
    ncols, ncells = 3000, 257
    cell, area = _ownership(ncols, ncells, 1)
    cell[cell == 7] = 8  # cell 7 left empty
    cell[np.arange(ncols) % 5 == 0] = 11  # one long cell (600 terms: past the vectorised phase)
    ptr, col, w = R.owner_map(cell, area, ncells)
    assert ptr[8] == ptr[7] and ptr[12] - ptr[11] >= 600
    rng = np.random.default_rng(2)
    x = rng.standard_normal((3, ncols)) * 1e3
    got = R.apply_aggregate(ptr, col, w, x, -999.0)
    assert got.shape == (3, ncells)
    for r in range(3):
        assert same_nan(got[r], loop_aggregate(ptr, col, w, x[r], -999.0))
        assert same_nan(R.apply_aggregate(ptr, col, w, x[r], -999.0), got[r])
    assert got[0, 7] == -999.0


def test_apply_aggregate_keeps_negative_zero_and_propagates_nan_and_inf():
    ptr = np.array([0, 1, 3, 3, 5, 7, 8])
    col = np.array([0, 1, 2, 3, 4, 5, 0, 6], np.int32)
    w = np.array([1.0, 0.5, 0.5, 2.0, 1.0, 0.25, 0.75, 1.0])
    x = np.array([-0.0, -0.0, -0.0, np.nan, 1.0, np.inf, 3.0])
    v = R.apply_aggregate(ptr, col, w, x, np.nan)
    assert v[0] == 0.0 and np.signbit(v[0])  # one term: -0.0 * 1.0
    assert v[1] == 0.0 and np.signbit(v[1])  # -0.0 + -0.0
    assert np.isnan(v[2])  # empty: fill
    assert np.isnan(v[3])  # NaN term
    assert v[4] == np.inf
    assert v[5] == 3.0
    assert same_nan(v, loop_aggregate(ptr, col, w, x, np.nan))
    # a map with no terms at all
    assert same_nan(R.apply_aggregate([0, 0, 0], [], [], x, 5.0), [5.0, 5.0])


def test_owner_map_weights_are_area_fractions():
    ncols, ncells = 20000, 700
    cell, area = _ownership(ncols, ncells, 3)
    ptr, col, w = R.owner_map(cell, area, ncells)
    assert ptr.dtype == np.int64 and col.dtype == np.int32 and ptr[0] == 0 and ptr[-1] == col.size == np.sum(cell >= 0)
    cnt = np.diff(ptr)
    for i in range(ncells):
        c = col[ptr[i]:ptr[i + 1]]
        assert np.all(np.diff(c) > 0)  # ascending columns
        assert np.all(cell[c] == i)
    live = cnt > 0
    assert not np.all(live) or ncells > 0
    sums = np.add.reduceat(w, ptr[:-1][live])
    np.testing.assert_allclose(sums, 1.0, rtol=0, atol=8 * np.finfo(float).eps)
    # a constant field maps to itself; area-weighted totals are conserved
    k = R.apply_aggregate(ptr, col, w, np.full(ncols, 287.15), np.nan)
    np.testing.assert_allclose(k[live], 287.15, rtol=8 * np.finfo(float).eps, atol=0)
    assert np.all(np.isnan(k[~live]))
    x = np.random.default_rng(4).random(ncols) * 400.0 - 50.0
    g = R.apply_aggregate(ptr, col, w, x, 0.0)
    area_cell = np.bincount(cell[cell >= 0], weights=area[cell >= 0], minlength=ncells)
    lhs, rhs = np.sum(area_cell * g), np.sum(area[cell >= 0] * x[cell >= 0])
    assert abs(lhs - rhs) <= 1e-13 * np.sum(np.abs(area * x))


def test_from_sparse_cells_orders_terms_by_column_per_cell():
    rng = np.random.default_rng(5)
    ncells, ncols, nnz = 50, 400, 1500
    row = rng.integers(0, ncells - 3, nnz)  # the last three cells stay empty
    col = rng.integers(0, ncols, nnz)
    S = rng.random(nnz)
    ptr, c, w = R.from_sparse_cells(row + 1, col + 1, S, ncells, ncols, one_based=True)
    assert ptr[0] == 0 and ptr[-1] == nnz and np.all(np.diff(ptr) >= 0) and np.all(np.diff(ptr)[-3:] == 0)
    for i in range(ncells):
        sel = np.nonzero(row == i)[0]
        want = sel[np.argsort(col[sel], kind="stable")]  # by column; repeated columns keep their file order
        assert np.array_equal(c[ptr[i]:ptr[i + 1]], col[want])
        assert np.array_equal(w[ptr[i]:ptr[i + 1]], S[want])
    x = rng.standard_normal(ncols)
    assert same_nan(R.apply_aggregate(ptr, c, w, x, -1.0), loop_aggregate(ptr, c, w, x, -1.0))


def test_slice_output_map_over_all_ranks_reproduces_the_global_result():
    ncols, ncells = 9001, 300
    rng = np.random.default_rng(6)
    # cell-contiguous columns (a spatial numbering), so most cells sit inside one rank's block; a few cells straddle
    cell = np.sort(rng.integers(0, ncells, ncols))
    cell[rng.random(ncols) < 0.01] = rng.integers(0, ncells)  # some strays
    area = rng.random(ncols) + 0.2
    ptr, col, w = R.owner_map(cell, area, ncells)
    x = rng.standard_normal(ncols) * 10.0
    want = R.apply_aggregate(ptr, col, w, x, np.nan)
    seen, strad = [], set()
    for rank in range(7):
        c0, n = decomp.block_range(ncols, 7, rank)
        pl, cl, wl, cells, straddling = R.slice_output_map(ptr, col, w, c0, n)
        assert pl.size == cells.size + 1 and np.all((cl >= 0) & (cl < n))
        assert same_nan(R.apply_aggregate(pl, cl, wl, x[c0:c0 + n], np.nan), want[cells])
        seen.append(cells)
        strad |= set(straddling.tolist())
    seen = np.concatenate(seen)
    assert np.unique(seen).size == seen.size  # every cell on at most one rank
    live = set(np.nonzero(np.diff(ptr) > 0)[0].tolist())
    assert set(seen.tolist()) | strad == live and not (set(seen.tolist()) & strad)
    assert 0 < len(strad) < ncells // 2
