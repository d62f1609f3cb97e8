"""Shortwave COSZEN mode on the device (include/elmk.h "shortwave"): czf against the reference's own average_cosz (oracle/_ref),
stepwise physics against the oracle, elmk_run against the stepwise calls (per-column series and a forcing grid, graph on and off),
conservation of each record's energy over its interval, the default left as it was, the refusals, and an exact restart."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import coszen_factor
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests import run_cases as GR
from tests.support import build_demo, run_demo, same, state_blob

pytestmark = pytest.mark.gpu

DT = GR.DT
FORC_DT = 3 * 3600.0  # 3-hourly records (GSWP3)
SPR = int(FORC_DT // DT)  # steps per record: 6
NSTEPS = 24
NREC = NSTEPS // SPR + 1  # slots 0 .. 4
DAY0 = 171.0  # records from 00:00 of the June solstice (decimal_doy)


def rec_times(nrec=NREC, day0=DAY0, forc_dt=FORC_DT):
    """Record starts as decimal_doy + 1.0, aligned on the day."""
    return day0 + 1.0 + np.arange(nrec) * forc_dt / 86400.0


def schedule(nsteps=NSTEPS, day0=DAY0):
    """Half-hour steps from 00:00 of day0 over 3-hourly records (slot s // 6), with run_cases' weights and months."""
    S = GR.schedule(nsteps)
    for s in range(nsteps):
        ddoy = day0 + s * DT / 86400.0
        S[s]["decday"] = ddoy + 1.0
        S[s]["doy"] = int(ddoy)
        S[s]["forc_slot"] = s // SPR
    return S


def stepwise(D, rec, steps, recs, history=False):
    """GR.stepwise with the record time of each step's record set before elmk_get_forcing."""
    cons, fo, fb = [], [], []
    for p in steps:
        D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
        f = int(p["forc_slot"])
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([rec[k][f], rec[k][f + 1]], axis=1))
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
        D.set_forcing_record_time(recs[f])
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"], False)
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        cons.append(st.kokkos_evaluate_conservation(D, DT))
        flags, first = D.error_summary()
        fo.append(flags)
        fb.append(first)
        if history:
            D.history_accumulate()
    return np.array(cons), np.array(fo, np.uint32), np.array(fb, np.int64)


def _coszen_device(base, graph=False):
    cols, scal, soil, lat, lon, rec = base
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.set_graph(graph)
    D.set_shortwave_mode("coszen", FORC_DT)
    return D


@pytest.fixture(scope="module")
def base():
    return GR._inputs(5003, 111, nrec=NREC)


def _ref_solar():
    from oracle import oracle as O

    if not O.have_ref() or not hasattr(O.Reference().R, "elmref_solar"):
        pytest.skip("oracle/_ref/libelmref.so not built (build() makes it where the reference is mounted)")
    R = O.Reference().R
    R.elmref_solar.argtypes = [C.c_int64] + [C.c_void_p] * 7
    R.elmref_solar.restype = None

    def cosz(lat, lon, dt, jday):
        n = lat.size
        a = [np.ascontiguousarray(np.broadcast_to(v, (n,)), dtype=np.float64) for v in (lat, lon, dt, jday)]
        out = [np.zeros(n) for _ in range(3)]
        R.elmref_solar(n, *[x.ctypes.data for x in a], *[o.ctypes.data for o in out])
        return out[0]

    return cosz


def test_czf_matches_the_reference_over_the_globe():
    """czf at 262 144 columns over the globe, bit for bit the reference's average_cosz(lat, lon, forc_dt, rec_decday), for 1, 3, 6
    and 24 h records at day 1, an equinox, a solstice and 365.875: through elmk_set_forcing_record_time and as the last step of a
    one-step run."""
    cosz = _ref_solar()
    n = 262_144
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=121)
    lat, lon = synth.global_grid(n, seed=122)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    D.run_reserve(2, 1)
    for k in st.SERIES_FORCING:
        D.series_upload(k, 0, cols[k].T)
    for k in st.SERIES_PHENOLOGY:
        D.series_upload(k, 0, np.repeat(cols[k][:, :1].T, 12, axis=0))
    for hours in (1, 3, 6, 24):
        forc_dt = hours * 3600.0
        D.set_shortwave_mode("coszen", forc_dt)
        for rec in (1.0, 80.5, 172.0, 365.875):
            want = cosz(lat, lon, forc_dt, rec)
            D.set_forcing_record_time(rec)
            assert same(D.forcing_cosz(), want), ("stepwise", hours, rec)
            step = schedule(1, day0=rec - 1.0)
            step[0]["forc_slot"] = 0
            D.series_record_times(0, [rec])
            D.run(DT, step)
            assert same(D.forcing_cosz(), want), ("run", hours, rec)
            if hours < 24:
                assert (want > 0).any() and (want == 0).any()
    D.close()


def test_stepwise_physics_matches_the_oracle():
    """Tier B, 40 000 columns on one latitude circle (one day length, every longitude): three steps of solar geometry, COSZEN
    get_forcing, init_timestep and advance_physics, against the oracle run with coszen := coszen_factor(cz, czf) for its
    get_forcing only: every field bit for bit."""
    n = 40_000
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=131)
    lat = np.full(n, 0.7)
    lon = (np.random.default_rng(132).random(n) - 0.5) * 2.0 * np.pi
    D = H.device_state(cols, scal, soil)
    D.set_column_geography(lat, lon)
    D.set_shortwave_mode("coszen", FORC_DT)
    S = None
    wt = np.random.default_rng(133).random(8)
    rec = DAY0 + 1.0 + 0.25  # the 06:00 record
    for s in range(3):
        decday = rec + s * DT / 86400.0
        D.solar_geometry(DT, decday, int(decday) - 1)
        D.set_forcing_record_time(rec)
        cz, czf = D["coszen"].reshape(-1).copy(), D.forcing_cosz()
        dayl, max_dayl = D.day_length()
        assert (dayl == dayl[0]).all() and (max_dayl == max_dayl[0]).all()
        if S is None:
            S = H.oracle_state(cols, dict(scal, dayl=float(dayl[0]), max_dayl=float(max_dayl[0])), soil)
        fac = coszen_factor(cz, czf)
        assert (fac > 1.0).any() and (fac < 1.0).any() and (fac == 0.0).any()
        st.compute_phenology(D, 0.3, 0.7)
        st.get_forcing(D, 1.0 - wt, wt, False)
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        S.phenology(0.3, 0.7)
        S["coszen"][...] = fac.reshape(S["coszen"].shape)
        S.get_forcing(1.0 - wt, wt, False)
        S["coszen"][...] = cz.reshape(S["coszen"].shape)
        S.init_timestep()
        S.timestep7(DT)
        S.soil_temperature(DT)
        S.snow_hydrology(DT)
        S.surface_fluxes(DT)
        worst, bad = H.compare_states(D, S, bitwise=True)
        assert not bad, (s, bad)
    D.close()


@pytest.mark.parametrize("graph", [True, False])
def test_run_equals_stepwise(base, graph):
    """24 half-hour steps over 3-hourly records as one elmk_run against the stepwise calls: every field, every conservation and flag
    ring row bit for bit."""
    cols, _, _, _, _, rec = base
    recs = rec_times()
    steps = schedule()
    A, B = _coszen_device(base, graph), _coszen_device(base, graph)
    want = stepwise(A, rec, steps, recs)
    B.run_reserve(NREC, NSTEPS)
    GR.upload_series(B, rec)
    B.series_record_times(0, recs)
    B.run(DT, steps)
    GR.assert_same_rows(B.run_diagnostics(), want)
    GR.assert_same_state(A, B, cols)
    assert same(A.forcing_cosz(), B.forcing_cosz())
    A.close()
    B.close()


@pytest.mark.parametrize("graph", [True, False])
def test_grid_run_equals_stepwise(base, graph):
    """The same over a bilinear forcing grid: a run over cell records against the stepwise calls fed the host remap of each record."""
    cols, scal, soil, lat, lon, rec = base
    nlon, nlat = 64, 32
    cells = {k: v for k, v in GR._inputs(nlon * nlat, 112, nrec=NREC)[-1].items() if k in st.SERIES_FORCING}
    idx, w = RG.bilinear_map(np.degrees(lat), np.degrees(lon), nlon, nlat)
    rec_cols = dict(rec)
    for k in st.SERIES_FORCING:
        rec_cols[k] = RG.apply_map(idx, w, cells[k])
    recs = rec_times()
    steps = schedule()
    A, B = _coszen_device(base, graph), _coszen_device(base, graph)
    want = stepwise(A, rec_cols, steps, recs)
    B.set_forcing_grid(idx, w, nlon * nlat)
    B.run_reserve(NREC, NSTEPS)
    for k in st.SERIES_FORCING:
        B.series_upload(k, 0, cells[k])
    for k in st.SERIES_PHENOLOGY:
        B.series_upload(k, 0, rec[k])
    B.series_record_times(0, recs)
    B.run(DT, steps)
    GR.assert_same_rows(B.run_diagnostics(), want)
    for name in A.fields:
        if name not in GR.SERIES:
            assert same(A[name], B[name]), name
    A.close()
    B.close()


def _band_sum(D):
    return D["forc_solad"].sum(axis=1) + D["forc_solai"].sum(axis=1)


def test_energy_of_each_record_is_kept(base):
    """Over each interval of six half-hour steps, the mean of sum_band (forc_solad + forc_solai) equals the record's FSDS within
    1e-11 relative on every column where no step had 0 < cz <= 0.001, none hit the cap and the interval's mean cos(zenith) czf is at
    least 0.01 (below it the reference's average_cosz is additive only to an absolute ~1e-13, tests/test_shortwave_host.py).  In
    REFERENCE mode the same mean is FSDS x the steps' mean cz: the gap COSZEN closes."""
    cols, scal, soil, lat, lon, rec = base
    recs = rec_times()
    fsds = rec["atm_fsds"]
    wt = np.zeros(8)
    for mode in ("coszen", "reference"):
        D = H.device_state(cols, scal, soil, lat=lat, lon=lon)
        D.set_shortwave_mode(mode, FORC_DT)
        for r in range(NREC - 1):
            D.upload("atm_fsds", np.stack([fsds[r], fsds[r + 1]], axis=1))
            tot, czs, ok = 0.0, 0.0, np.ones(D.ncols, bool)
            for s in range(SPR):
                decday = recs[r] + s * DT / 86400.0
                D.solar_geometry(DT, decday, int(decday) - 1)
                if mode == "coszen":
                    D.set_forcing_record_time(recs[r])
                    czf = D.forcing_cosz()
                st.get_forcing(D, 1.0 - wt, wt, False)
                cz = D["coszen"].reshape(-1)
                tot = tot + _band_sum(D)
                czs = czs + cz
                if mode == "coszen":
                    ok &= ~((cz > 0.0) & (cz <= 0.001)) & ~(cz / np.where(czf > 0, czf, 1.0) >= 10.0) & (czf >= 0.01)
            mean = tot / SPR
            if mode == "coszen":
                assert ok.sum() > D.ncols // 4, r
                err = np.abs(mean[ok] - fsds[r][ok])
                assert (err <= 1e-11 * np.abs(fsds[r][ok])).all(), (r, float((err / np.abs(fsds[r][ok])).max()))
            else:
                want = fsds[r] * (czs / SPR)
                assert np.allclose(mean, want, rtol=1e-12, atol=1e-12), r
                lit = (czs > 0) & (fsds[r] > 0)
                assert lit.any() and (mean[lit] < fsds[r][lit]).all()  # the placeholder never delivers the record
        D.close()


def test_reference_mode_is_the_default(base):
    """A context switched COSZEN -> REFERENCE runs bit-identical to a fresh one; a context that only set REFERENCE allocates
    nothing more."""
    cols, scal, soil, lat, lon, rec = base
    steps = GR.schedule()
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    A.set_graph(True)
    B.set_graph(True)
    bytes_fresh = B.device_bytes
    B.set_shortwave_mode("reference")
    assert B.device_bytes == bytes_fresh
    B.set_shortwave_mode("coszen", FORC_DT)
    assert B.device_bytes == bytes_fresh + B.level_stride * 8  # czf
    start = {k: A[k] for k in A.fields}
    for D in (A, B):
        D.run_reserve(GR.NREC, GR.NSTEPS)
        GR.upload_series(D, rec)
    B.series_record_times(0, rec_times(GR.NREC))
    B.run(DT, steps[:2])  # a COSZEN run, captured
    B.set_shortwave_mode("reference")
    # B has run two COSZEN steps: back to the state A starts from
    for k, v in start.items():
        B.upload(k, v)
    A.run(DT, steps)
    B.run(DT, steps)
    GR.assert_same_rows(A.run_diagnostics(), B.run_diagnostics())
    for name in A.fields:
        assert same(A[name], B[name]), name
    A.close()
    B.close()


def test_refusals_leave_everything_as_it_was(base):
    """Every refusal is ELMK_E_INVALID and changes nothing; times are forgotten by elmk_run_reserve, a forcing grid and a change of
    mode or forc_dt."""
    cols, scal, soil, lat, lon, rec = base
    n = cols["t_grnd"].shape[0]
    lib = L.load()
    recs = rec_times()
    steps = schedule(12)

    def rc(f, *a):
        return getattr(lib, f)(D.ctx, *a)

    D = st.ELMState(n)  # no geography
    assert rc("elmk_set_shortwave_mode", 1, FORC_DT) == -1
    assert rc("elmk_set_forcing_record_time", 172.0) == -1  # REFERENCE mode
    D.close()

    D = _coszen_device(base)
    czf_ptr = np.zeros(n)
    assert rc("elmk_download_forcing_cosz", czf_ptr.ctypes.data_as(C.c_void_p)) == -1  # nothing computed yet
    for bad in (0.0, -1.0, np.nan, np.inf, 86400.0 * 366.0 + 1.0):
        assert rc("elmk_set_shortwave_mode", 1, bad) == -1, bad
    assert rc("elmk_set_shortwave_mode", 2, FORC_DT) == -1
    assert rc("elmk_set_shortwave_mode", -1, FORC_DT) == -1
    assert rc("elmk_set_shortwave_mode", 1, 86400.0 * 366.0) == 0  # the bound itself is accepted
    assert rc("elmk_set_shortwave_mode", 1, FORC_DT) == 0
    # stepwise: no record time yet, a bad time
    w = np.zeros(8)
    assert rc("elmk_get_forcing", w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0) == -1
    for bad in (-1.0, np.nan, np.inf, 1e9):
        assert rc("elmk_set_forcing_record_time", bad) == -1
    # runs: no reservation, slots out of range, bad times, a step without a time
    t = np.array(recs)
    tp = t.ctypes.data_as(C.c_void_p)
    assert rc("elmk_series_record_times", 0, NREC, tp) == -1
    D.run_reserve(NREC, NSTEPS)
    GR.upload_series(D, base[5])
    assert rc("elmk_series_record_times", -1, 1, tp) == -1
    assert rc("elmk_series_record_times", 1, NREC, tp) == -1
    assert rc("elmk_series_record_times", 0, 1, None) == -1
    tb = np.array([172.0, np.nan])
    assert rc("elmk_series_record_times", 0, 2, tb.ctypes.data_as(C.c_void_p)) == -1
    assert rc("elmk_series_record_times", 0, 1, tp) == 0  # slot 0 only
    S = np.ascontiguousarray(steps)
    run = lambda: rc("elmk_run", C.c_double(DT), S.ctypes.data_as(C.c_void_p), len(S), 0)  # noqa: E731
    assert run() == -1  # steps 6 .. 11 read slot 1 (and the refused NaN time set none)
    before = {k: D[k] for k in D.fields}
    assert rc("elmk_series_record_times", 0, NREC, tp) == 0
    # forgotten: by a change of forc_dt, of mode, by elmk_run_reserve, by a forcing grid
    for forget in ("forc_dt", "mode", "reserve", "grid"):
        if forget == "forc_dt":
            D.set_shortwave_mode("coszen", 2 * FORC_DT)
            D.set_shortwave_mode("coszen", FORC_DT)
        elif forget == "mode":
            D.set_shortwave_mode("reference")
            D.set_shortwave_mode("coszen", FORC_DT)
        elif forget == "reserve":
            D.run_reserve(NREC, NSTEPS)
            GR.upload_series(D, base[5])
        else:
            idx, wg = RG.nearest_map(np.degrees(lat), np.degrees(lon), 8, 4)
            D.set_forcing_grid(idx, wg, 32)
            D.clear_forcing_grid()
            D.run_reserve(NREC, NSTEPS)
            GR.upload_series(D, base[5])
        assert run() == -1, forget
        assert rc("elmk_get_forcing", w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0) == -1, forget
        assert rc("elmk_series_record_times", 0, NREC, tp) == 0
    for k, v in before.items():
        assert same(D[k], v), k
    # clearing the geography goes back to REFERENCE: get_forcing needs no record time again
    D.clear_column_geography()
    assert rc("elmk_get_forcing", w.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), 0) == 0
    assert rc("elmk_series_record_times", 0, NREC, tp) == -1
    D.close()


def test_exact_restart_in_coszen_mode(base):
    """2N steps give the bits of N steps, save, load into a fresh context (mode and times set again), then N steps."""
    from elmkernels_amd import restart as RS

    cols, scal, soil, lat, lon, rec = base
    recs = rec_times()
    steps = schedule()
    half = NSTEPS // 2
    A = _coszen_device(base, graph=True)
    A.run_reserve(NREC, NSTEPS)
    GR.upload_series(A, rec)
    A.series_record_times(0, recs)
    A.run(DT, steps)
    B = _coszen_device(base, graph=True)
    B.run_reserve(NREC, NSTEPS)
    GR.upload_series(B, rec)
    B.series_record_times(0, recs)
    B.run(DT, steps[:half])
    img = B.restart_save()
    B.close()
    RS.verify(img)
    Cx = _coszen_device(base, graph=True)
    GR.poison(Cx)
    Cx.run_reserve(NREC, NSTEPS)
    Cx.restart_load(img)
    GR.upload_series(Cx, rec)
    Cx.series_record_times(0, recs)
    Cx.run(DT, steps[half:])
    for name in A.fields:
        if name not in GR.SERIES:
            assert same(A[name], Cx[name]), name
    assert same(A.forcing_cosz(), Cx.forcing_cosz())
    A.close()
    Cx.close()


def test_shortwave_demo_runs(tmp_path):
    """examples/shortwave_demo.cc compiles with g++ against the C ABI and runs 48 half-hour steps over 3-hourly records whose FSDS is
    1000 W/m2 x czf (no sunlight where the sun stays down): in COSZEN mode the day's mean incident shortwave is the records' mean
    (within 1 %: the 0.001 threshold and the cap), in REFERENCE mode it falls short."""
    exe = build_demo("shortwave_demo", tmp_path)
    n, nrec, nsteps = 3008, 2 * NSTEPS // SPR + 1, 2 * NSTEPS
    cols, scal, soil, lat, lon, rec = GR._inputs(n, 141, nrec=nrec)
    recs = rec_times(nrec)
    G = st.ELMState(n)
    G.set_column_geography(lat, lon)
    G.set_shortwave_mode("coszen", FORC_DT)
    for r in range(nrec):
        G.set_forcing_record_time(recs[r])
        rec["atm_fsds"][r] = 1000.0 * G.forcing_cosz()
    G.close()
    extra = GR.demo_records(lat, lon, rec) + [("recs", recs), ("steps", schedule(nsteps))]
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, extra))
    out = run_demo(exe, tmp_path / "state.bin")
    print(out.stdout)
    assert "coszen: kept" in out.stdout and "reference: short" in out.stdout, out.stdout
