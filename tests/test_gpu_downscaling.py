"""Downscaling of coarse-grid forcing to column elevation on the device (include/elmk.h "downscaling"): equal elevations give the
bits of OFF, elmk_get_forcing in TOPO mode against elmkernels_amd/downscale.py (with the oracle's qsat), elmk_run against the
stepwise calls (per-column series and a forcing grid, graph on and off), the physical properties of the adjusted fields, the snow a
mountain column keeps, the refusals, an exact restart and the demo; and the longwave renormalisation on its own (k_ds_lw_norm) on
every group shape of tests/output_map_cases.py, in both builds."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import downscale as DSC
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests import helpers as H
from tests import output_map_cases as OM
from tests import run_cases as GR
from tests.support import build_demo, captured, run_demo, same, same_nan, state_blob

pytestmark = pytest.mark.gpu

DT = GR.DT
NSTEPS = 24
NREC = NSTEPS // 2 + 1  # GR.schedule: slot s // 2
DS_FIELDS = ("forc_tbot", "forc_thbot", "forc_pbot", "forc_qbot", "forc_lwrad", "forc_rain", "forc_snow")
KEPT_FIELDS = ("forc_solad", "forc_solai", "forc_u", "forc_v", "forc_hgt", "forc_hgt_u_patch", "forc_hgt_t_patch", "forc_hgt_q_patch")
NLON, NLAT = 64, 32


@pytest.fixture(scope="module")
def base():
    return GR._inputs(5003, 211, nrec=NREC)


def _qsat():
    """The oracle's qsat (elmo_qsat, the reference's qsat_impl.hh restated and pinned to it bit for bit): (T, p) -> qs."""
    from oracle import oracle as O

    return lambda T, p: O.qsat(T, p)[2]


def test_oracle_qsat_is_the_references():
    """Where oracle/_ref is built: the qsat these tests use has the bits of the reference's own, over both clamps of td."""
    from oracle import oracle as O

    if not O.have_ref():
        pytest.skip("oracle/_ref/libelmref.so not built (build() makes it where the reference is mounted)")
    rng = np.random.default_rng(7)
    T = rng.uniform(180.0, 390.0, 20000)
    p = rng.uniform(4.0e4, 1.05e5, 20000)
    for a, b in zip(O.qsat(T, p), O.Reference().qsat(T, p)):
        assert same(a, b)


def _elevations(n, seed):
    """hf: a forcing surface height per column; hc within +-1500 m of it, equal to it on every tenth column."""
    rng = np.random.default_rng(seed)
    hf = 200.0 + 1500.0 * rng.random(n)
    hc = hf + rng.uniform(-1500.0, 1500.0, n)
    hc[::10] = hf[::10]
    return hc, hf


def _groups(n, seed):
    """regrid.owner_map with ~150 columns per group, 19 columns in no group and the last column a group of its own."""
    cell = np.arange(n) // 150
    cell[n - 20:n - 1] = -1
    cell[n - 1] = cell.max() + 1
    area = 0.5 + np.random.default_rng(seed).random(n)
    return RG.owner_map(cell, area, int(cell.max()) + 1)


def _col(D, k):
    return D[k].reshape(-1).copy()


def _forcing(D):
    return {k: D[k] for k in DS_FIELDS + KEPT_FIELDS}


def _topo_device(base, hc, hf, groups=None, graph=False, mode="topo"):
    cols, scal, soil, lat, lon, rec = base
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_graph(graph)
    D.set_column_elevation(hc, hf)
    if groups is not None:
        D.set_downscaling_groups(*groups)
    D.set_downscaling(mode)
    return D


@pytest.mark.parametrize("path", ["stepwise", "run_graph", "run"])
def test_equal_elevations_give_the_bits_of_off(base, path):
    """TOPO with topo_col == topo_forc (random heights) and longwave groups: every field, conservation and flag row of 24 steps has
    the bits of OFF."""
    cols = base[0]
    n = cols["t_grnd"].shape[0]
    h = 100.0 + 3000.0 * np.random.default_rng(5).random(n)
    steps = GR.schedule(NSTEPS)
    graph = path == "run_graph"
    A = _topo_device(base, h, h, graph=graph, mode="off")
    B = _topo_device(base, h, h, groups=_groups(n, 6), graph=graph)
    if path == "stepwise":
        GR.assert_same_rows(GR.stepwise(B, base[5], steps), GR.stepwise(A, base[5], steps))
    else:
        for D in (A, B):
            D.run_reserve(NREC, NSTEPS)
            GR.upload_series(D, base[5])
            D.run(DT, steps)
        GR.assert_same_rows(B.run_diagnostics(), A.run_diagnostics())
    for name in A.fields:
        assert same(A[name], B[name]), name
    A.close()
    B.close()


@pytest.mark.parametrize("grid,rh,sw,groups", [
    (False, False, "reference", False),
    (False, False, "reference", True),
    (False, True, "coszen", True),
    (False, True, "reference", False),
    (True, False, "coszen", False),
    (True, True, "reference", True),
    (True, False, "reference", True),
])
def test_stepwise_matches_the_host_restatement(base, grid, rh, sw, groups):
    """elmk_get_forcing in TOPO mode writes, bit for bit, downscale.py applied to the same step's OFF values; shortwave, wind and
    heights keep the OFF bits.  Grid: the records and hf come through a bilinear forcing grid (hf by
    elmk_set_forcing_elevation_gridded, bit for bit regrid.apply_map)."""
    qsat = _qsat()
    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    rng = np.random.default_rng(17)
    hc, hf = _elevations(n, 18)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    if grid:
        ncells = NLON * NLAT
        idx, w = RG.bilinear_map(np.degrees(lat), np.degrees(lon), NLON, NLAT)
        cells = GR._inputs(ncells, 112, nrec=2)[-1]
        D.set_forcing_grid(idx, w, ncells)
        for k in st.SERIES_FORCING:
            D.upload_gridded(k, cells[k][0], level=0)
            D.upload_gridded(k, cells[k][1], level=1)
        hcells = 200.0 + 1500.0 * rng.random(ncells)
        D.set_column_elevation(hc)
        D.set_forcing_elevation_gridded(hcells)
        hf = RG.apply_map(idx, w, hcells)
    else:
        D.set_column_elevation(hc, hf)
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([rec[k][0], rec[k][1]], axis=1))
    got_hc, got_hf = D.column_elevation()
    assert same(got_hc, hc) and same(got_hf, hf)
    D.solar_geometry(DT, 172.3, 171)
    if sw == "coszen":
        D.set_shortwave_mode("coszen", 3 * 3600.0)
        D.set_forcing_record_time(172.25)
    wt = rng.random(8)
    st.get_forcing(D, 1.0 - wt, wt, rh)
    off = _forcing(D)
    prec = D["atm_prec"][:, 0].copy()
    G = _groups(n, 19) if groups else None
    if G is not None:
        D.set_downscaling_groups(*G)
    D.set_downscaling("topo")
    st.get_forcing(D, 1.0 - wt, wt, rh)
    got = _forcing(D)
    want = DSC.downscale_forcing(off, prec, hc, hf, qsat, groups=G)
    for k in DS_FIELDS:
        assert same(got[k], want[k]), k
    for k in KEPT_FIELDS:
        assert same(got[k], off[k]), k
    moved = hc != hf
    assert (got["forc_tbot"][moved] != off["forc_tbot"][moved]).all()
    assert same(got["forc_tbot"][~moved], off["forc_tbot"][~moved])
    if G is not None:  # the single-column group gives back Lg (to rounding)
        c = n - 1
        assert abs(got["forc_lwrad"][c] - off["forc_lwrad"][c]) <= 4 * np.spacing(off["forc_lwrad"][c])
    D.close()


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("graph", [True, False])
def test_run_equals_stepwise(base, grid, graph):
    """24 TOPO steps with longwave groups as one elmk_run against the stepwise calls: every field, conservation and flag row bit for
    bit; over per-column series, and over cell series of a bilinear forcing grid with hf from the grid."""
    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    hc, hf = _elevations(n, 21)
    G = _groups(n, 22)
    steps = GR.schedule(NSTEPS)
    if not grid:
        A = _topo_device(base, hc, hf, G, graph)
        B = _topo_device(base, hc, hf, G, graph)
        want = GR.stepwise(A, rec, steps)
        B.run_reserve(NREC, NSTEPS)
        GR.upload_series(B, rec)
    else:
        ncells = NLON * NLAT
        idx, w = RG.bilinear_map(np.degrees(lat), np.degrees(lon), NLON, NLAT)
        cells = {k: v for k, v in GR._inputs(ncells, 113, nrec=NREC)[-1].items() if k in st.SERIES_FORCING}
        hcells = 200.0 + 1500.0 * np.random.default_rng(23).random(ncells)
        rec_cols = dict(rec)
        for k in st.SERIES_FORCING:
            rec_cols[k] = RG.apply_map(idx, w, cells[k])
        A = _topo_device(base, hc, RG.apply_map(idx, w, hcells), G, graph)
        want = GR.stepwise(A, rec_cols, steps)
        B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
        B.set_graph(graph)
        B.set_forcing_grid(idx, w, ncells)
        B.set_column_elevation(hc)
        B.set_forcing_elevation_gridded(hcells)
        B.set_downscaling_groups(*G)
        B.set_downscaling("topo")
        B.run_reserve(NREC, NSTEPS)
        for k in st.SERIES_FORCING:
            B.series_upload(k, 0, cells[k])
        for k in st.SERIES_PHENOLOGY:
            B.series_upload(k, 0, rec[k])
    B.run(DT, steps)
    GR.assert_same_rows(B.run_diagnostics(), want)
    for name in A.fields:
        if name not in GR.SERIES:
            assert same(A[name], B[name]), name
    A.close()
    B.close()


def test_physical_properties(base):
    """On the device's output: tc - tg = -lapse dz to rounding, relative humidity kept (qc / qs_c = qg / qs_g to 1e-15), rain + snow
    = prec to 1 ulp (2 ulp at most, the split's roundings), Lc inside the lw_limit band without groups, and with groups each group's weighted mean of Lc that of Lg to 1e-13."""
    qsat = _qsat()
    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    hc, hf = _elevations(n, 31)
    G = _groups(n, 32)
    lapse, lapse_lw, lw_limit = 0.0065, 0.05, 0.3
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_column_elevation(hc, hf)
    for k in st.SERIES_FORCING:
        D.upload(k, np.stack([rec[k][0], rec[k][1]], axis=1))
    D.solar_geometry(DT, 172.3, 171)
    wt = np.full(8, 0.4)
    st.get_forcing(D, 1.0 - wt, wt, False)
    off = _forcing(D)
    prec = np.maximum(D["atm_prec"][:, 0], 0.0)
    D.set_downscaling("topo", lapse, lapse_lw, lw_limit)
    st.get_forcing(D, 1.0 - wt, wt, False)
    got = _forcing(D)
    dz = hc - hf
    tg, tc = off["forc_tbot"], got["forc_tbot"]
    assert (np.abs((tc - tg) + lapse * dz) <= 2 * np.spacing(tg)).all()
    qg, qc = off["forc_qbot"], got["forc_qbot"]
    rh_g = qg / qsat(tg, off["forc_pbot"])
    rh_c = qc / qsat(tc, got["forc_pbot"])
    assert (np.abs(rh_c - rh_g) <= 1e-15 * rh_g).all()
    tot = got["forc_rain"] + got["forc_snow"]  # three roundings in the split and one in this sum
    assert (np.abs(tot - prec) <= 2 * np.spacing(prec)).all()
    assert (np.abs(tot - prec) <= np.spacing(prec)).mean() > 0.99
    lg, lc = off["forc_lwrad"], got["forc_lwrad"]
    assert (lc >= lg * (1.0 - lw_limit)).all() and (lc <= lg * (1.0 + lw_limit)).all()
    assert (got["forc_pbot"][dz > 0] < off["forc_pbot"][dz > 0]).all() and (got["forc_pbot"][dz < 0] > off["forc_pbot"][dz < 0]).all()
    D.set_downscaling_groups(*G)
    st.get_forcing(D, 1.0 - wt, wt, False)
    lcn = _col(D, "forc_lwrad")
    ptr, col, w = G
    ones = np.ones(n)
    mean_g = RG.apply_aggregate(ptr, col, w, lg, 0.0) / RG.apply_aggregate(ptr, col, w, ones, 0.0)
    mean_c = RG.apply_aggregate(ptr, col, w, lcn, 0.0) / RG.apply_aggregate(ptr, col, w, ones, 0.0)
    assert (np.abs(mean_c - mean_g) <= 1e-13 * mean_g).all()
    free = np.setdiff1d(np.arange(n), col)
    assert free.size == 19 and same(lcn[free], lc[free])  # columns of no group are not renormalised
    D.close()


F32_GROUP_SHAPES = (("tiles", 33), ("big_last", 17), ("tile_start", 33), ("all_empty", 33))
GROUP_SHAPES = ([(n, layout, None) for layout in OM.LAYOUTS for n in OM.GROUP_NCELLS]
                + [(n, layout, L.F32_LIB_PATH) for layout, n in F32_GROUP_SHAPES])


@pytest.mark.parametrize("ncells,layout,lib_path", GROUP_SHAPES, ids=lambda v: "f32" if v == L.F32_LIB_PATH else "f64" if v is None else None)
def test_group_renormalisation_on_every_group_shape(ncells, layout, lib_path):
    """k_ds_lw_norm on its own, at the shapes its two walks and its search can go wrong at (output_map_cases.shape_map with 16
    groups per workgroup, every column in at most one group): 1, 15, 16, 17 and 33 groups; a workgroup span of exactly one tile and
    of one tile and a column, a group of more than two tiles, a workgroup without a column, groups that start exactly at a tile's
    start, no column at all; an empty group, a
    one-column group, a group whose weights are all 0.0 (W == 0), a group led by a NaN Lg, a NaN in a column of no group.  OFF gives
    Lg, TOPO without groups gives the Lc the kernel reads, TOPO with groups must give downscale.renormalise_longwave(Lg, Lc) bit
    for bit.  In libelmk_f32.so Lg is the widened record itself (weights 1 and 0, no computed column) and the result is the fp64
    product rounded once to fp32.  No qsat is needed: every other field is compared with the TOPO call before the groups."""
    f32 = lib_path is not None
    cnt = OM.cell_counts(ncells, 61, layout, OM.DS_CELLS)[0]
    n1 = int((cnt == 1).sum())
    # column 0 leads the first group of two or more columns that shape_map gives away (columns 1 .. n1 lead the one-column groups)
    lead = tuple(range(1, n1 + 1)) + (0,) if OM.edge_columns(ncells, layout)[0] else ()
    ptr, col, w, ncols = OM.shape_map(ncells, 61, layout, cells_per_wg=OM.DS_CELLS, disjoint=True, lead=lead)
    assert (np.diff(ptr) == cnt).all()
    nan_lead = lead[-1:]
    cols, scal, soil, lat, lon, rec = GR._inputs(ncols, 62, nrec=2)
    hc, hf = _elevations(ncols, 63)
    rng = np.random.default_rng(64)
    flds = rng.uniform(60.0, 590.0, (2, ncols))
    computed = np.zeros(ncols, bool)
    if f32:
        flds = flds.astype(np.float32).astype(np.float64)
    else:  # every 13th column: both records outside [50, 600], so the interpolated one is too and lwrad is computed
        computed[::13] = True
        flds[:, computed] = np.where(np.arange(computed.sum()) % 2 == 0, 30.0, 700.0)
    free = np.setdiff1d(np.arange(ncols), col)
    nan_cols = [int(free[0])] + list(nan_lead)
    flds[0, nan_cols] = np.nan
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    D.set_column_elevation(hc, hf)
    for k in st.SERIES_FORCING:
        D.upload(k, np.stack([rec[k][0], rec[k][1]], axis=1))
    D.upload("atm_flds", np.stack([flds[0], flds[1]], axis=1))
    D.solar_geometry(DT, 172.3, 171)
    wt2 = rng.random(8)
    if f32:
        wt2[3] = 0.0
    wt1 = 1.0 - wt2
    # 1. OFF: Lg
    st.get_forcing(D, wt1, wt2, False)
    lg = _col(D, "forc_lwrad")
    if f32:
        assert wt1[3] == 1.0 and same_nan(lg, flds[0].astype(np.float32).astype(np.float64))
        lg = flds[0].copy()  # exact: 1.0 * record 0 + 0.0 * record 1; the device keeps it in fp64, the download rounds it
    else:
        interp = flds[0] * wt1[3] + flds[1] * wt2[3]
        assert ((interp[computed] <= 50.0) | (interp[computed] >= 600.0) | np.isnan(interp[computed])).all()
        plain = ~computed & ~np.isnan(interp)
        assert same(lg[plain], interp[plain]) and (lg[computed & ~np.isnan(interp)] != interp[computed & ~np.isnan(interp)]).all()
    assert np.isnan(lg[nan_cols]).all() and np.isnan(lg).sum() == len(nan_cols)
    # 2. TOPO without groups: the Lc the kernel reads
    D.set_downscaling("topo")
    st.get_forcing(D, wt1, wt2, False)
    before = _forcing(D)
    lc = before["forc_lwrad"].reshape(-1).copy()
    assert (np.isnan(lc) == np.isnan(lg)).all() and (lc[hc != hf] != lg[hc != hf])[~np.isnan(lg[hc != hf])].any()
    # 3. with the groups
    D.set_downscaling_groups(ptr, col, w)
    st.get_forcing(D, wt1, wt2, False)
    got = _forcing(D)
    out = got["forc_lwrad"].reshape(-1)
    with np.errstate(all="ignore"):
        norm = DSC.group_norm(lg, lc, ptr, col, w)
        if f32:
            want = lc.copy()
            want[col] = (lc[col] * np.repeat(norm, cnt)).astype(np.float32).astype(np.float64)
        else:
            want = DSC.renormalise_longwave(lg, lc, ptr, col, w)
    bad = np.nonzero(~((out.view(np.uint64) == want.view(np.uint64)) | (np.isnan(out) & np.isnan(want))))[0]
    group_of = np.full(ncols, -1, np.int64)
    group_of[col] = np.repeat(np.arange(ncells), cnt)
    assert not bad.size, (bad[:5].tolist(), group_of[bad[:5]].tolist(), out[bad[:5]].tolist(), want[bad[:5]].tolist(), norm[group_of[bad[:5]]].tolist())
    # by value
    assert same(out[free], lc[free]) and free.size >= 3  # a column of no group keeps its bits, the NaN among them
    W = RG.apply_aggregate(ptr, col, w, np.ones(ncols), 0.0)
    zero, _, own = OM.special_cells(cnt)
    unit = np.isin(group_of, np.nonzero(W == 0.0)[0])  # W == 0: the norm is exactly 1
    assert same(out[unit], lc[unit])
    if layout == "all_empty":
        assert same(out, lc) and not col.size
    else:
        live = (W > 0.0) & ~np.isnan(norm)
        assert live.any() and (norm[live] != 1.0).any() and (out[col] != lc[col]).any()
    if zero is not None:
        assert W[zero] == 0.0 and cnt[zero] >= 2 and unit[col[ptr[zero]]]
    new_nan = np.isnan(out) & ~np.isnan(lc)
    if nan_lead:
        g = own[n1]
        assert group_of[0] == g and cnt[g] >= 2 and np.isnan(norm[g]) and np.isnan(out[col[ptr[g]:ptr[g + 1]]]).all()
        assert (group_of[new_nan] == g).all() and new_nan.sum() == cnt[g] - 1  # no other group took a NaN
    else:
        assert not new_nan.any()
    for k in DS_FIELDS + KEPT_FIELDS:
        if k != "forc_lwrad":
            assert same(got[k], before[k]), k
    # once more: the same bits (forc_lwrad is rewritten by the forcing kernel first, so the norm does not compound)
    st.get_forcing(D, wt1, wt2, False)
    assert same(D["forc_lwrad"], got["forc_lwrad"])
    D.close()


def _snow_case(n, seed, nrec=25):
    """Identical columns (the state of one synthetic column, one position) under identical near-freezing records: 275 K, wet,
    at night; even columns at the cell's surface height (800 m), odd columns 1 500 m above it."""
    cols, scal, soil, lat, lon, rec = GR._inputs(n, seed, nrec=nrec)
    cols = {k: np.repeat(v[:1], n, axis=0) for k, v in cols.items()}
    lat, lon = np.full(n, lat[0]), np.full(n, lon[0])
    const = {"atm_tbot": 275.0, "atm_pbot": 85000.0, "atm_qbot": 0.004, "atm_flds": 300.0, "atm_fsds": 0.0, "atm_prec": 1.0e-3,
             "atm_wind": 3.0}
    for k in st.SERIES_FORCING:
        rec[k] = np.full((nrec, n), const[k])
    for k in st.SERIES_PHENOLOGY:
        rec[k] = np.repeat(rec[k][:, :1], n, axis=1)
    hf = np.full(n, 800.0)
    hc = np.where(np.arange(n) % 2 == 0, 800.0, 2300.0)
    return (cols, scal, soil, lat, lon, rec), hc, hf


def test_mountain_columns_keep_more_snow():
    """48 steps of near-freezing forcing from one cell: columns 1 500 m above the cell's surface end with more h2osno than columns at
    its height in TOPO mode (their precipitation falls as snow); with downscaling OFF every column ends alike."""
    n = 256
    case, hc, hf = _snow_case(n, 301)
    out = {}
    for mode in ("off", "topo"):
        D = _topo_device(case, hc, hf, graph=True, mode=mode)
        D.run_reserve(25, 48)
        GR.upload_series(D, case[5])
        D.run(DT, GR.schedule(48))
        out[mode] = _col(D, "h2osno")
        D.close()
    valley, mountain = slice(0, None, 2), slice(1, None, 2)
    h = out["off"]
    assert (h == h[0]).all()
    h = out["topo"]
    assert (h[mountain] > h[valley]).all() and (h[mountain] > out["off"][mountain]).all(), (h[valley][:3], h[mountain][:3])


def test_refusals_enqueue_nothing(base):
    """Every refusal is ELMK_E_INVALID and leaves the context as a twin that made only the valid calls: the same forcing bits after a
    TOPO step and the same device bytes.  A context that never downscales allocates nothing more."""
    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    hc, hf = _elevations(n, 41)
    G = _groups(n, 42)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)  # refusals
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)  # twin
    bytes0 = A.device_bytes

    def P(a):
        return np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)

    def rc(f, *a):
        return getattr(A.lib, f)(A.ctx, *a)

    good = (0.006, 0.032, 0.5)
    assert rc("elmk_set_downscaling", 1, *good) == -1  # no elevations
    assert rc("elmk_set_forcing_elevation_gridded", P(np.zeros(8))) == -1  # no forcing map
    bad_hc = hc.copy()
    bad_hc[7] = np.nan
    assert rc("elmk_set_column_elevation", P(bad_hc), P(hf)) == -1
    bad_hf = hf.copy()
    bad_hf[3] = np.inf
    assert rc("elmk_set_column_elevation", P(hc), P(bad_hf)) == -1
    assert rc("elmk_set_column_elevation", None, P(hf)) == -1
    assert A.device_bytes == bytes0
    A.set_column_elevation(hc)  # hc only: TOPO still refused
    assert rc("elmk_set_downscaling", 1, *good) == -1
    A.set_column_elevation(hc, hf)
    for mode, p in [(2, good), (-1, good), (1, (np.nan, 0.032, 0.5)), (1, (0.006, np.inf, 0.5)), (1, (0.006, 0.032, np.nan)),
                    (1, (-1e-3, 0.032, 0.5)), (1, (0.006, -1e-3, 0.5)), (1, (0.006, 0.032, -0.1)), (1, (0.006, 0.032, 1.0))]:
        assert rc("elmk_set_downscaling", mode, *p) == -1, (mode, p)
    ptr, col, w = G
    ptr = np.ascontiguousarray(ptr, np.int64)
    col = np.ascontiguousarray(col, np.int32)
    w = np.ascontiguousarray(w, np.float64)

    def groups_rc(p, c, ww, ng=None):
        return rc("elmk_set_downscaling_groups", C.c_int64(p.size - 1 if ng is None else ng), P(p), P(c), P(ww))

    c2 = col.copy()
    c2[200] = c2[10]  # a column in two groups
    assert groups_rc(ptr, c2, w) == -1
    assert A.lib.elmk_last_error(A.ctx) == b"elmk_set_downscaling_groups: a column in more than one group (or twice in one)"
    for v in (-0.1, np.nan, np.inf):
        w2 = w.copy()
        w2[5] = v
        assert groups_rc(ptr, col, w2) == -1, v
    for v in (-1, n):
        c3 = col.copy()
        c3[3] = v
        assert groups_rc(ptr, c3, w) == -1, v
    p2 = ptr.copy()
    p2[0] = 1
    assert groups_rc(p2, col, w) == -1
    p3 = ptr.copy()
    p3[2] = p3[1] - 1
    assert groups_rc(p3, col, w) == -1
    assert groups_rc(ptr, col, w, ng=0) == -1
    # valid calls, then refusals under capture of each setter
    A.set_downscaling_groups(*G)
    A.set_downscaling("topo", 0.0065, 0.04, 0.4)
    with captured(A):
        refused = [rc("elmk_set_column_elevation", P(hf), P(hc)) == -1,
                   rc("elmk_set_downscaling", 0, *good) == -1,
                   rc("elmk_set_downscaling_groups", C.c_int64(1), P(np.array([0, 1], np.int64)), P(np.array([0], np.int32)), P(np.ones(1))) == -1,
                   rc("elmk_clear_downscaling_groups") == -1,
                   rc("elmk_download_column_elevation", P(np.zeros(n)), None) == -1]
    assert all(refused), refused
    # the twin
    B.set_column_elevation(hc, hf)
    B.set_downscaling_groups(*G)
    B.set_downscaling("topo", 0.0065, 0.04, 0.4)
    assert A.device_bytes == B.device_bytes > bytes0
    for D in (A, B):
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([rec[k][0], rec[k][1]], axis=1))
        D.solar_geometry(DT, 172.3, 171)
        st.get_forcing(D, np.full(8, 0.5), np.full(8, 0.5), False)
    for name in A.fields:
        assert same(A[name], B[name]), name
    A.close()
    B.close()


def test_exact_restart_in_topo_mode(base):
    """N steps, save, load into a fresh context with the same downscaling setup, N steps: the bits of 2N steps."""
    from elmkernels_amd import restart as RS

    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    hc, hf = _elevations(n, 51)
    G = _groups(n, 52)
    steps = GR.schedule(NSTEPS)
    half = NSTEPS // 2
    A = _topo_device(base, hc, hf, G, graph=True)
    A.run_reserve(NREC, NSTEPS)
    GR.upload_series(A, rec)
    A.run(DT, steps)
    B = _topo_device(base, hc, hf, G, graph=True)
    B.run_reserve(NREC, NSTEPS)
    GR.upload_series(B, rec)
    B.run(DT, steps[:half])
    img = B.restart_save()
    B.close()
    RS.verify(img)
    Cx = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    Cx.set_graph(True)
    GR.poison(Cx)
    Cx.set_column_elevation(hc, hf)
    Cx.set_downscaling_groups(*G)
    Cx.set_downscaling("topo")
    Cx.run_reserve(NREC, NSTEPS)
    Cx.restart_load(img)
    GR.upload_series(Cx, rec)
    Cx.run(DT, steps[half:])
    for name in A.fields:
        if name not in GR.SERIES:
            assert same(A[name], Cx[name]), name
    A.close()
    Cx.close()


def test_downscaling_demo(tmp_path):
    """examples/downscaling_demo.cc compiles with g++ against the C ABI and runs a day of valley and mountain columns in one forcing
    cell: with downscaling OFF they end alike, in TOPO mode the mountain is colder and keeps more snow."""
    exe = build_demo("downscaling_demo", tmp_path)
    n = 512
    (cols, scal, soil, lat, lon, rec), hc, hf = _snow_case(n, 311)
    extra = GR.demo_records(lat, lon, rec) + [("topo", hc), ("hf", hf[:1]), ("steps", GR.schedule(48))]
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, extra))
    out = run_demo(exe, tmp_path / "state.bin")
    print(out.stdout)
    assert "off: valley and mountain alike" in out.stdout and "topo: more snow on the mountain" in out.stdout, out.stdout
