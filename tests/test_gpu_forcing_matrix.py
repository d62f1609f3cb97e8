"""Every kernel body of k_forcing.hip against one host reference (tests/forcing_cases.py: reference, none of it device output), bit
for bit, NaN positions included, on edge inputs, at 1, 256, 257 and 1001 columns, in libelmk.so and libelmk_f32.so:

  stepwise   elmk_get_forcing in its four modes (REFERENCE / COSZEN x OFF / TOPO, TOPO with and without longwave groups), specific and
             relative humidity, weights (1, 0) and general ones; and behind elmk_upload_gridded / elmk_set_forcing_elevation_gridded at
             every map width 1 .. 8 (k_remap_field<N>, k_remap_field_f64<N> and the host's padding of 3, 5, 6, 7);
  runs       three steps of elmk_run over per-column series (k_get_forcing_run*) and over cell series of every width 1, 2, 4, 8 in
             every mode (k_get_forcing_run_grid*<N>; 3 and 7 padded), the forcing of EVERY step captured by the point series;
  phenology  k_phenology and k_phenology_run against the oracle's phenology.

tests/test_forcing_cases_host.py shows without a GPU that these inputs take both sides of every branch."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests import forcing_cases as FC
from tests import helpers as H
from tests import run_cases as GR
from tests.support import same, same_nan

pytestmark = pytest.mark.gpu

LIBS = {"f64": None, "f32": L.F32_LIB_PATH}
BUILDS = ["f64", "f32"]
SIZES = (1, 256, 257, 1001)
RUN_SIZES = (257, 1001)
MODES = ("reference", "coszen", "topo", "coszen_topo")
NCELLS = 37
REC_DAY = 172.25  # stepwise: the record of 06:00 on the June solstice
NSLOTS = 7
RUN_SLOTS = (0, 3, NSLOTS - 2)  # slot 0, a middle slot, the last pair (NSLOTS - 2, NSLOTS - 1)
RUN_REC_DAYS = 172.0 + 0.125 * np.arange(NSLOTS)  # 3-hourly records from midnight
RUN_DECDAYS = (172.02, 172.44, 172.70)  # the steps: night / dawn / afternoon somewhere; not all inside their record's interval (the cap)
PHEN_FIELDS = ("tlai", "tsai", "htop", "hbot", "elai", "esai", "frac_veg_nosno_alb")


# ---- shared inputs: computed once, never changed -----------------------------------------------------------------------------------
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _base(n):
    """State, geography and phenology months of n columns (run_cases._inputs)."""
    return _cached(("base", n), lambda: GR._inputs(n, 700 + n, nrec=2))


def _edge(n):
    return _cached(("edge", n), lambda: FC.edge_records(n, 900 + n, nrec=NSLOTS))


def _map(width, n):
    return _cached(("map", width, n), lambda: FC.edge_map(width, n, NCELLS, 40 + width))


def _cells(width, n):
    sp = _map(width, n)[2]
    return _cached(("cells", width, n), lambda: (FC.edge_cells(NCELLS, 50 + width, sp, nrec=NSLOTS), FC.edge_heights(NCELLS, 60 + width, sp)))


def _device(n, build, graph=True):
    cols, scal, soil, _, _, _ = _base(n)
    E = _edge(n)
    D = H.device_state(cols, scal, soil, lat=E["lat"], lon=E["lon"], lib_path=LIBS[build])
    D.set_graph(graph)
    return D


def _forc(D):
    return {k: D[k] for k in FC.FORC_FIELDS}


def _assert_forcing(got, want, what, fields=FC.FORC_FIELDS):
    for k in fields:
        g, w = np.ascontiguousarray(got[k], dtype=np.float64), np.ascontiguousarray(want[k], dtype=np.float64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        ok = (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
        assert ok.all(), (what, k, int((~ok).sum()), np.argwhere(~ok)[:3].tolist(), g[~ok][:3].tolist(), w[~ok][:3].tolist())


def _set_mode(D, E, mode, groups=False, hcells=None):
    """The shortwave and downscaling modes of `mode`; TOPO with E's elevations, the forcing's from the grid's cells where hcells is given."""
    if "coszen" in mode:
        D.set_shortwave_mode("coszen", FC.FORC_DT)
    else:
        D.set_shortwave_mode("reference")
    if "topo" in mode:
        if hcells is None:
            D.set_column_elevation(E["hc"], E["hf"])
        else:
            D.set_column_elevation(E["hc"])
            D.set_forcing_elevation_gridded(hcells)
        if groups:
            D.set_downscaling_groups(*E["groups"])
        D.set_downscaling("topo", FC.LAPSE, FC.LAPSE_LW, FC.LW_LIMIT)


def _stepwise_coszen(E):
    """(cz, czf) of the stepwise tests: czf of the 06:00 record on the host, cz with every special planted against it."""
    czf = FC.cosz_host(E["lat"], E["lon"], FC.FORC_DT, REC_DAY)
    return FC.edge_coszen(czf, 5)[0], czf


# ---- stepwise ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_stepwise_matches_the_reference(n, mode, build):
    """k_get_forcing, k_get_forcing_cz, k_get_forcing_ds<false>, k_get_forcing_ds<true>: every forc_* row (the forc_hgt_*_patch rows
    among them, which stay as the forcing kernel left them here), for specific and relative humidity, under weights (1, 0) - the
    planted values reach their thresholds exactly - and general weights, TOPO without and with the longwave groups."""
    E = _edge(n)
    f32 = build == "f32"
    D = _device(n, build)
    cz, czf = _stepwise_coszen(E)
    D["coszen"] = cz
    for with_groups in ((False, True) if "topo" in mode else (False,)):
        _set_mode(D, E, mode, groups=with_groups)
        if "coszen" in mode:
            D.set_forcing_record_time(REC_DAY)
            assert same(D.forcing_cosz(), czf), "czf of the device against the host build of elmk_solar.h"
        if "topo" in mode:
            hc, hf = D.column_elevation()
            assert same(hc, E["hc"]) and same(hf, E["hf"])
        for rh in (False, True):
            rec = FC.rec_for(E, rh)
            for k in FC.STREAMS:
                D.upload(k, np.stack([rec[k][0], rec[k][1]], axis=1))
            for kind in ("exact", "general"):
                wt = FC.edge_weights(kind, 11)
                st.get_forcing(D, wt[0], wt[1], rh)
                want = FC.reference(rec, wt, rh, cz, czf=czf if "coszen" in mode else None,
                                    topo=FC.topo_of(E) if "topo" in mode else None, groups=E["groups"] if with_groups else None, f32=f32)
                _assert_forcing(_forc(D), want, (mode, "groups" if with_groups else "no groups", "rh" if rh else "q", kind))
    D.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_stepwise_behind_gridded_uploads_at_every_width(n, build):
    """k_remap_field<1, 2, 4, 8> (elmk_upload_gridded, both levels of every stream) and k_remap_field_f64<1, 2, 4, 8>
    (elmk_set_forcing_elevation_gridded, read back with column_elevation) at every width 1 .. 8 of the edge map over 37 cells whose
    unreferenced cells hold NaN: the uploaded records equal regrid.apply_map bit for bit, and the forcing step behind them the
    reference, in REFERENCE mode and with COSZEN and TOPO on."""
    E = _edge(n)
    f32 = build == "f32"
    r32 = FC.f32_round if f32 else (lambda a: a)
    D = _device(n, build)
    cz, czf = _stepwise_coszen(E)
    D["coszen"] = cz
    wt = FC.edge_weights("general", 12)
    for width in range(1, 9):
        idx, w, _ = _map(width, n)
        cells, hcells = _cells(width, n)
        D.set_shortwave_mode("reference")
        D.set_forcing_grid(idx, w, NCELLS)
        rec = {k: cells[k][:2] for k in FC.STREAMS}
        for k in FC.STREAMS:
            D.upload_gridded(k, rec[k][0], level=0)
            D.upload_gridded(k, rec[k][1], level=1)
        for k in FC.STREAMS:
            got = D[k]
            for lev in (0, 1):
                assert same(got[:, lev], r32(RG.apply_map(idx, w, rec[k][lev]))), (width, k, lev)
        D.set_column_elevation(E["hc"])
        D.set_forcing_elevation_gridded(hcells)
        hc, hf = D.column_elevation()
        assert same(hc, E["hc"]) and same(hf, RG.apply_map(idx, w, hcells)), width
        assert np.isfinite(hf).all()
        D.set_downscaling("off")
        st.get_forcing(D, wt[0], wt[1], False)
        want = FC.reference(rec, wt, False, cz, grid=(idx, w), f32=f32, stored_remap=True)
        _assert_forcing(_forc(D), want, (width, "reference"))
        _set_mode(D, E, "coszen_topo", groups=True, hcells=hcells)
        D.set_forcing_record_time(REC_DAY)
        st.get_forcing(D, wt[0], wt[1], False)
        want = FC.reference(rec, wt, False, cz, grid=(idx, w), czf=czf, topo=FC.topo_of(E, hcells), groups=E["groups"], f32=f32,
                            stored_remap=True)
        _assert_forcing(_forc(D), want, (width, "coszen_topo"))
        for k in FC.FORC_FIELDS:
            assert np.isfinite(want[k]).all(), (width, k)
        D.set_downscaling("off")
    D.close()


# ---- runs ----------------------------------------------------------------------------------------------------------------------------
def _steps(rh):
    """Three steps: forcing slots 0, 3 and the last pair; weights (1, 0), then two distinct general sets; month brackets (11, 0), (11, 0),
    (0, 1)."""
    S = GR.schedule(3)
    for s in range(3):
        S[s]["decday"] = RUN_DECDAYS[s]
        S[s]["doy"] = int(RUN_DECDAYS[s]) - 1
        S[s]["forc_slot"] = RUN_SLOTS[s]
        wt = FC.edge_weights("exact" if s == 0 else "general", 20 + s)
        S[s]["forc_wt1"], S[s]["forc_wt2"] = wt
    S[2]["month1"], S[2]["month2"], S[2]["month_wt1"], S[2]["month_wt2"] = 0, 1, 0.85, 1.0 - 0.85
    return S


def _arm_points(D, n, rows):
    D.points_set("columns", np.arange(n))
    ids = [D.points_add_field(name, lev) for name, lev in rows]
    D.points_reserve(3)
    D.points_set_run(True)
    return ids


def _recorded(D, ids, rows, s):
    """{field: [n] or [n, 2]} of record s."""
    out = {}
    for e, (name, lev) in zip(ids, rows):
        v = D.points_read(e, s, 1)[0]
        if D.fields[name][1] == 1:
            out[name] = v
        else:
            out.setdefault(name, np.zeros((v.size, D.fields[name][1])))[:, lev] = v
    return out


RUN_ROWS = FC.FORC_ROWS + (("coszen", 0),)
WRITTEN = tuple(k for k in FC.FORC_FIELDS if k not in FC.HGT_PATCH)  # (init_timestep rewrites the patch heights later in the step)


def _run_case(n, build, mode, rh, width, graph, twin=False):
    """Three steps of elmk_run in `mode` over per-column series (width None) or over cell series behind the edge map of `width` rows;
    every step's forc_* rows, as the point series recorded them, against the reference of that step."""
    E = _edge(n)
    f32 = build == "f32"
    cols, scal, soil, _, _, base_rec = _base(n)
    steps = _steps(rh)
    flags = st.RUN_QBOT_IS_RH if rh else 0
    D = _device(n, build, graph)
    grid = None
    if width is None:
        series = dict(E["rec"], atm_qbot=E["rh"] if rh else E["rec"]["atm_qbot"])
        hf = None
    else:
        idx, w, _ = _map(width, n)
        cells, hf = _cells(width, n)
        series = dict(cells)
        if rh:  # per cent, as tests/test_gpu_parity.py makes them (a NaN cell stays NaN)
            series["atm_qbot"] = np.clip(cells["atm_qbot"] * 4000.0, 0.0, 100.0)
        grid = (idx, w)
        D.set_forcing_grid(idx, w, NCELLS)
    _set_mode(D, E, mode, groups="topo" in mode, hcells=hf)
    D.run_reserve(NSLOTS, 3)
    for k in FC.STREAMS:
        D.series_upload(k, 0, series[k])
    for k in st.SERIES_PHENOLOGY:
        D.series_upload(k, 0, base_rec[k])
    if "coszen" in mode:
        D.series_record_times(0, RUN_REC_DAYS)
    ids = _arm_points(D, n, RUN_ROWS)
    D.run(FC.DT, steps, flags)
    assert D.points_count() == (3, 3)
    seen = []
    for s, p in enumerate(steps):
        slot = int(p["forc_slot"])
        got = _recorded(D, ids, RUN_ROWS, s)
        cz = FC.cosz_host(E["lat"], E["lon"], FC.DT, float(p["decday"]))
        assert same(got["coszen"], FC.f32_round(cz) if f32 else cz), (s, "coszen of the step against the host build of elmk_solar.h")
        czf = FC.cosz_host(E["lat"], E["lon"], FC.FORC_DT, RUN_REC_DAYS[slot]) if "coszen" in mode else None
        rec = {k: series[k][slot:slot + 2] for k in FC.STREAMS}
        want = FC.reference(rec, (p["forc_wt1"], p["forc_wt2"]), rh, cz, grid=grid, czf=czf,
                            topo=FC.topo_of(E, hf) if "topo" in mode else None, groups=E["groups"] if "topo" in mode else None, f32=f32)
        _assert_forcing(got, want, (mode, "step", s, "slot", slot), WRITTEN)
        seen.append(got)
    assert not same(seen[0]["forc_tbot"], seen[1]["forc_tbot"]) or n == 1
    if twin:  # the patch heights: what the stepwise chain leaves after each step
        A = _device(n, build, graph)
        _set_mode(A, E, mode, groups="topo" in mode)
        left = []
        GR.stepwise(A, dict(base_rec, **series), steps, flags, dt=FC.DT, rec_times=RUN_REC_DAYS if "coszen" in mode else None,
                    per_step=(left, lambda X: {k: X[k] for k in FC.HGT_PATCH}))
        for s in range(3):
            for k in FC.HGT_PATCH:
                assert same_nan(seen[s][k], left[s][k]), (s, k)
        A.close()
    D.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("rh", [False, True], ids=["q", "rh"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SIZES)
def test_run_over_column_series_matches_the_reference(n, mode, rh, build):
    """k_get_forcing_run, k_get_forcing_run_cz, k_get_forcing_run_ds<false>, k_get_forcing_run_ds<true>.  At 257 columns the recorded
    forc_hgt_*_patch rows also equal what the stepwise chain of the same steps leaves."""
    _run_case(n, build, mode, rh, None, True, twin=n == 257 and not rh)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width", (1, 2, 4, 8))
@pytest.mark.parametrize("n", RUN_SIZES)
def test_run_over_cell_series_matches_the_reference(n, width, mode, build):
    """k_get_forcing_run_grid<N>, k_get_forcing_run_grid_cz<N>, k_get_forcing_run_grid_ds<N, false>, k_get_forcing_run_grid_ds<N,
    true> for N = 1, 2, 4, 8: the sixteen bodies, over 37 cells (no multiple of the level stride) whose unreferenced cells hold NaN.
    Widths 2 and 8 run the relative-humidity stream."""
    _run_case(n, build, mode, width in (2, 8), width, True)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("width", (1, 2, 4, 8))
@pytest.mark.parametrize("n", RUN_SIZES)
def test_run_over_cell_series_without_the_graph(n, width, build):
    """COSZEN, TOPO and the forcing grid all on at once, launched directly instead of replayed from the captured graph."""
    _run_case(n, build, "coszen_topo", width in (2, 8), width, False)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("width", (3, 7))
def test_run_over_cell_series_of_padded_widths(width, build):
    """Maps of 3 and 7 rows, which the host pads to 4 and 8, with COSZEN and TOPO on."""
    _run_case(257, build, "coszen_topo", False, width, True)


# ---- phenology -------------------------------------------------------------------------------------------------------------------------
def _phenology_want(S, Ph, months, m1, m2, wt1, snow_depth, frac_sno, r32):
    for k in st.SERIES_PHENOLOGY:
        S[k][:, 0], S[k][:, 1] = r32(months[k][m1]), r32(months[k][m2])
    S["vtype"][:] = Ph["vtype"]
    S["snow_depth"][:] = r32(snow_depth)
    S["frac_sno"][:] = r32(frac_sno)
    S.phenology(wt1, 1.0 - wt1)
    return {k: (S[k].copy() if S[k].dtype != np.float64 else r32(S[k])) for k in PHEN_FIELDS}


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", SIZES)
def test_phenology_matches_the_oracle(n, build):
    """k_phenology for the month pairs (11, 0) and (0, 1), then k_phenology_run in three steps of elmk_run (each step's snow_depth and
    frac_sno are the previous step's, recorded by the point series): vtype 0, 1, 11, 12 and 14, snow below, inside and above the
    canopy and around 0.2 m, leaf and stem areas on both sides of 0.05."""
    from oracle import oracle as O

    f32 = build == "f32"
    r32 = FC.f32_round if f32 else (lambda a: np.asarray(a, dtype=np.float64))
    cols, scal, soil, _, _, base_rec = _base(n)
    E = _edge(n)
    Ph = FC.edge_phenology(n, 80 + n)
    months = Ph["months"]
    D = _device(n, build)
    D["vtype"] = Ph["vtype"]
    D["snow_depth"] = Ph["snow_depth"]
    D["frac_sno"] = Ph["frac_sno"]
    S = O.OracleState(n)
    for (m1, m2), wt1 in (((11, 0), 0.3), ((0, 1), 0.85)):
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([months[k][m1], months[k][m2]], axis=1))
        st.compute_phenology(D, wt1, 1.0 - wt1)
        want = _phenology_want(S, Ph, months, m1, m2, wt1, Ph["snow_depth"], Ph["frac_sno"], r32)
        _assert_forcing({k: D[k] for k in PHEN_FIELDS}, want, ("stepwise", m1, m2), PHEN_FIELDS)
    # the run
    steps = _steps(False)
    D.run_reserve(NSLOTS, 3)
    for k in FC.STREAMS:
        D.series_upload(k, 0, E["rec"][k])
    for k in st.SERIES_PHENOLOGY:
        D.series_upload(k, 0, months[k])
    rows = tuple((k, 0) for k in PHEN_FIELDS + ("snow_depth", "frac_sno"))
    ids = _arm_points(D, n, rows)
    D.run(FC.DT, steps, 0)
    snow, fsno = r32(Ph["snow_depth"]), r32(Ph["frac_sno"])
    for s, p in enumerate(steps):
        got = _recorded(D, ids, rows, s)
        want = _phenology_want(S, Ph, months, int(p["month1"]), int(p["month2"]), float(p["month_wt1"]), snow, fsno, r32)
        assert float(p["month_wt2"]) == 1.0 - float(p["month_wt1"])
        _assert_forcing(got, want, ("run", s), PHEN_FIELDS)
        snow, fsno = got["snow_depth"], got["frac_sno"]
    D.close()
