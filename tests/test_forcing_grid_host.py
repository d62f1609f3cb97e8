"""Forcing on a coarser grid without a GPU: the map builders and apply_map of elmkernels_amd/regrid.py, and the C ABI of include/elmk.h
("forcing grid") declared, in the ctypes table and exported by both builds."""
import re
import os

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import decomp
from elmkernels_amd import regrid as R
from tests.support import ROOT

NLON, NLAT = 64, 32


def _columns(n, seed):
    rng = np.random.default_rng(seed)
    lat = np.degrees(np.arcsin(2.0 * rng.random(n) - 1.0))
    lon = (rng.random(n) - 0.5) * 360.0
    return lat, lon


def _centres(nlon=NLON, nlat=NLAT, lon0=0.0):
    i, j = np.arange(nlon), np.arange(nlat)
    lonc = lon0 + (i + 0.5) * 360.0 / nlon
    latc = -90.0 + (j + 0.5) * 180.0 / nlat
    return np.tile(lonc, nlat), np.repeat(latc, nlon)  # cell = j * nlon + i


def test_bilinear_weights_sum_to_one_and_are_in_range():
    lat, lon = _columns(20000, 1)
    idx, w = R.bilinear_map(lat, lon, NLON, NLAT)
    assert idx.shape == w.shape == (4, 20000) and idx.dtype == np.int32
    assert np.all((idx >= 0) & (idx < NLON * NLAT))
    assert np.all((w >= 0.0) & (w <= 1.0))
    np.testing.assert_allclose(w.sum(axis=0), 1.0, rtol=0, atol=4e-16)


def test_bilinear_reproduces_a_field_linear_in_lat_lon():
    """Inside the band of cell centres and away from the dateline, a field linear in longitude and latitude is interpolated exactly
    (to rounding)."""
    rng = np.random.default_rng(2)
    n = 5000
    lat = rng.uniform(-90.0 + 180.0 / NLAT, 90.0 - 180.0 / NLAT, n)  # between the outermost centre rows
    lon = rng.uniform(360.0 / NLON, 360.0 - 360.0 / NLON, n)  # between the first and the last centre column
    lonc, latc = _centres()
    field = 0.25 * lonc - 1.5 * latc + 7.0
    idx, w = R.bilinear_map(lat, lon, NLON, NLAT)
    np.testing.assert_allclose(R.apply_map(idx, w, field), 0.25 * lon - 1.5 * lat + 7.0, rtol=0, atol=1e-11)


def test_bilinear_wraps_at_the_dateline_and_clamps_at_the_poles():
    dlon = 360.0 / NLON
    # just east of 0 (before the first centre) and just west of 360: between cells nlon-1 and 0, weight by distance
    idx, w = R.bilinear_map(np.array([0.1, 0.1]), np.array([0.25 * dlon, 360.0 - 0.25 * dlon]), NLON, NLAT)
    j0 = idx[0] // NLON
    for c in range(2):
        assert set(idx[[0, 1], c] % NLON) == {NLON - 1, 0}
        assert np.all(idx[:, c] // NLON >= j0[c])
    wi = {int(idx[k, 0] % NLON): 0.0 for k in range(4)}
    for k in range(4):
        wi[int(idx[k, 0] % NLON)] += w[k, 0]
    np.testing.assert_allclose([wi[NLON - 1], wi[0]], [0.25, 0.75], atol=1e-15)
    # the same longitude expressed as -180 .. 180 gives the same map
    i2, w2 = R.bilinear_map(np.array([0.1]), np.array([-0.25 * dlon]), NLON, NLAT)
    assert np.array_equal(i2[:, 0], idx[:, 1]) and np.array_equal(w2[:, 0], w[:, 1])
    # on and beyond the poles: the polar centre row only
    idx, w = R.bilinear_map(np.array([90.0, -90.0, 89.99]), np.array([10.0, 10.0, 10.0]), NLON, NLAT)
    field = np.repeat(np.arange(NLAT, dtype=np.float64), NLON)  # = the row
    assert np.array_equal(R.apply_map(idx, w, field), [NLAT - 1, 0, NLAT - 1])


def test_land_mask_renormalises_over_land_corners():
    lat, lon = _columns(4000, 3)
    rng = np.random.default_rng(4)
    land = rng.random(NLON * NLAT) < 0.6
    idx0, w0 = R.bilinear_map(lat, lon, NLON, NLAT)
    idx, w = R.bilinear_map(lat, lon, NLON, NLAT, land=land)
    assert np.all(idx[0] >= 0)  # row 0 is never padding
    on0 = land[idx0]
    some = np.any(on0 & (w0 > 0), axis=0)
    # a column with a land corner of positive weight reads land cells only, weights renormalised
    real = idx >= 0
    assert np.all(land[np.where(real, idx, 0)][:, some] | ~real[:, some])
    np.testing.assert_allclose(w[:, some].sum(axis=0), 1.0, atol=4e-16)
    for c in np.nonzero(some)[0][:200]:
        m = on0[:, c]
        want = dict(zip(idx0[m, c], w0[m, c] / w0[m, c].sum()))
        got = dict(zip(idx[real[:, c], c], w[real[:, c], c]))
        assert got.keys() == want.keys()
        np.testing.assert_allclose([got[k] for k in want], list(want.values()), rtol=1e-15)
    # padding terms carry weight 0 and sit behind the real ones
    assert np.all(w[~real] == 0.0)
    assert np.all(np.diff(real.astype(int), axis=0) <= 0)
    # a column without land around it keeps the unmasked weights
    idx1, w1 = R.bilinear_map(np.array([0.0]), np.array([10.0]), NLON, NLAT, land=np.zeros(NLON * NLAT, bool))
    i2, w2 = R.bilinear_map(np.array([0.0]), np.array([10.0]), NLON, NLAT)
    assert np.array_equal(idx1, i2) and np.array_equal(w1, w2)


def test_nearest_map_picks_the_containing_cell():
    lat, lon = _columns(20000, 5)
    idx, w = R.nearest_map(lat, lon, NLON, NLAT)
    assert idx.shape == (1, 20000) and np.all(w == 1.0)
    i, j = idx[0] % NLON, idx[0] // NLON
    lon_w = np.mod(lon, 360.0)
    dlon, dlat = 360.0 / NLON, 180.0 / NLAT
    assert np.all((i * dlon <= lon_w) & (lon_w < (i + 1) * dlon))
    assert np.all((-90.0 + j * dlat <= lat) & (lat <= -90.0 + (j + 1) * dlat))
    # poles and the dateline
    idx, _ = R.nearest_map(np.array([90.0, -90.0, 0.0, 0.0]), np.array([180.0, -180.0, 360.0, -1e-9]), NLON, NLAT)
    assert list(idx[0] // NLON) == [NLAT - 1, 0, NLAT // 2, NLAT // 2]
    assert list(idx[0] % NLON)[2:] == [0, NLON - 1]


def test_from_sparse_orders_terms_and_pads():
    # column 0: cells 7, 2, 5 (unsorted); column 1: one cell; column 2: cells 3, 1
    row = np.array([0, 2, 0, 1, 0, 2])
    col = np.array([7, 3, 2, 4, 5, 1])
    S = np.array([0.1, 0.6, 0.2, 1.0, 0.7, 0.4])
    idx, w = R.from_sparse(row, col, S, ncols=3, ncells=8)
    assert idx.dtype == np.int32 and idx.shape == (3, 3)
    assert idx.tolist() == [[2, 4, 1], [5, -1, 3], [7, -1, -1]]
    assert w.tolist() == [[0.2, 1.0, 0.4], [0.7, 0.0, 0.6], [0.1, 0.0, 0.0]]
    i1, w1 = R.from_sparse(row + 1, col + 1, S, ncols=3, ncells=8, one_based=True)
    assert np.array_equal(i1, idx) and np.array_equal(w1, w)
    with pytest.raises(ValueError):
        R.from_sparse(row, col, S, ncols=4, ncells=8)  # column 3 has no term
    with pytest.raises(ValueError):
        R.from_sparse(np.zeros(9, int), np.arange(9), np.ones(9), ncols=1, ncells=9)  # 9 terms
    with pytest.raises(ValueError):
        R.from_sparse(row, col, S, ncols=3, ncells=7)  # cell 7 out of range


def test_slice_map_over_all_ranks_reassembles_the_remap():
    lat, lon = _columns(10007, 6)
    land = np.random.default_rng(7).random(NLON * NLAT) < 0.7
    idx, w = R.bilinear_map(lat, lon, NLON, NLAT, land=land)
    cells = np.random.default_rng(8).standard_normal((3, NLON * NLAT))
    want = R.apply_map(idx, w, cells)
    for world in (1, 3, 8):
        parts = []
        for col0, n in decomp.all_ranges(idx.shape[1], world):
            il, wl, used = R.slice_map(idx, w, col0, n)
            assert il.shape == (4, n) and np.all(il[0] >= 0) and np.all(il < used.size)
            assert np.all(np.diff(used) > 0)
            parts.append(R.apply_map(il, wl, cells[:, used]))
        got = np.concatenate(parts, axis=1)
        assert got.tobytes() == want.tobytes()


def test_apply_map_skips_padding_and_keeps_negative_zero():
    cells = np.array([-0.0, np.nan, 3.0, np.inf, -0.0])
    idx = np.array([[0, 2, 4], [-1, 1, -1], [-1, -1, 0]], np.int32)
    w = np.array([[1.0, 0.5, 2.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    v = R.apply_map(idx, w, cells)
    assert np.signbit(v[0]) and v[0] == 0.0  # -0.0 alone: no + 0.0 * a
    assert np.isnan(v[1])  # a real term (weight 0) on a NaN cell is read
    assert v[2] == 0.0 and np.signbit(v[2])  # -0.0 + -0.0
    idx[1, 1] = -1
    assert R.apply_map(idx, w, cells)[1] == 1.5  # the NaN cell behind padding is never read
    idx2 = np.array([[3], [-1]], np.int32)
    assert R.apply_map(idx2, np.array([[1.0], [0.0]]), cells)[0] == np.inf
    # the operation order: ((w0*a0 + w1*a1) + w2*a2), not a dot product in another order
    a = np.array([1.0, 1e16, -1e16])
    i3 = np.array([[1], [2], [0]], np.int32)
    assert R.apply_map(i3, np.ones((3, 1)), a)[0] == 1.0
    assert R.apply_map(np.array([[0], [1], [2]], np.int32), np.ones((3, 1)), a)[0] == 0.0
    # several records at once
    recs = np.stack([cells, cells * 2])
    assert R.apply_map(idx, w, recs).shape == (2, 3)


def test_forcing_grid_abi_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "elmk.h")).read()
    declared = {"elmk_set_forcing_grid", "elmk_clear_forcing_grid", "elmk_upload_gridded"}
    assert declared <= set(re.findall(r"^int (elmk_\w+)\(", header, re.M))
    assert declared <= set(L.SIGNATURES)
    for path in (L.LIB_PATH, L.F32_LIB_PATH):
        lib = L.load(path)
        for name in declared:
            assert getattr(lib, name) is not None
