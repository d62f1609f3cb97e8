"""Oracle restatement vs the REFERENCE ITSELF (oracle/_ref/libelmref.so = the reference's own headers,
compiled by oracle/Makefile from /root/reference) on seeded synthetic columns that reach the branches the
bundled fixtures never take: snow layers 1..5, bare ground, capped snow, ponded water, all snowfall regimes.

Same compiler family, same libm, same operation order => the bar here is bit-for-bit equality.
Skipped (not failed) where the reference library was not built (it cannot be built on the GPU box, but the
prebuilt .so travels there).
"""
import numpy as np
import pytest

from elmkernels_amd import synth
from oracle import oracle as O
from tests import helpers as H

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/libelmref.so not built here")

N = 4096


@pytest.fixture(scope="module")
def states():
    ft = H.field_table_from_oracle()
    cols, scal, soil = synth.make_state(ft, N, tier="B", seed=1234)
    A = H.oracle_state(cols, scal, soil)
    B = A.clone()
    return A, B


def test_branch_coverage_of_the_synthetic_state(states):
    A, _ = states
    assert set(np.unique(A["snl"])) == {0, 1, 2, 3, 4, 5}
    assert (A["frac_veg_nosno"] == 0).any() and (A["frac_veg_nosno"] == 1).any()
    assert A["do_capsnow"].any() and (A["h2osfc"] > 1e-8).any()
    assert (A["coszen"] > 0).any() and (A["coszen"] <= 0).any()
    t = A["forc_tbot"]
    assert (t > 275.15).any() and ((t > 258.15) & (t <= 275.15)).any() and (t <= 258.15).any()


def test_five_wrappers_bit_exact_vs_reference(states):
    """frac_wet, canopy_hydrology, surface_radiation, canopy_temperature, bareground_fluxes in timestep order."""
    A, B = states
    R = O.Reference()
    A.frac_wet(); R.frac_wet(B)
    assert not H.oracle_diffs(A, B)
    A.canopy_hydrology(1800.0); R.canopy_hydrology(B, 1800.0)
    assert not H.oracle_diffs(A, B)
    # albedo products come from the oracle on both sides here (the albedo wrapper by the reference's own functions, and all
    # seven wrappers chained by the reference alone: tests/test_oracle_vs_ref_canopy.py)
    A.albedo_snicar()
    for k in A.fields:
        B.fields[k][...] = A.fields[k]
    A.surface_radiation(); R.surface_radiation(B)
    d = H.oracle_diffs(A, B, [k for k in A.fields if k != "err_flags"])
    assert not d, d
    A.canopy_temperature(); R.canopy_temperature(B)
    d = H.oracle_diffs(A, B, [k for k in A.fields if k != "err_flags"])
    assert not d, d
    A.bareground_fluxes(); R.bareground_fluxes(B)
    d = H.oracle_diffs(A, B, [k for k in A.fields if k != "err_flags"])
    assert not d, d
    # the new-snow-layer branch of snow_init must have fired somewhere
    assert (A["snl"] == 1).sum() > 0


def test_snicar_bit_exact_vs_reference():
    ft = H.field_table_from_oracle()
    cols, scal, soil = synth.make_state(ft, N, tier="B", seed=99)
    A = H.oracle_state(cols, scal, soil)
    A.albedo_snicar()  # oracle: full wrapper; leaves albsoi/albsod in the state for the reference run
    B = A.clone()
    B["albsnd"][:] = -1.0
    B["albsni"][:] = -1.0
    R = O.Reference()
    fd, fi = R.snicar(B)
    assert not (B["err_flags"] & (1 << 31)).any()  # the reference threw nowhere
    assert not (A["err_flags"] & 0x7FF).any()
    # albsnd/albsni: direct outputs of both SNICAR passes
    assert np.array_equal(A["albsnd"], B["albsnd"]) and np.array_equal(A["albsni"], B["albsni"])
    # the per-layer absorption factors reach the state through flux_absorption_factor (subgridflag == 1):
    # flx_absdv = flx_absd_snw(:,0) * (1 - albsnd(0)) etc. (surface_albedo_impl.hh:200-206)
    day = A["coszen"] > 0
    for name, f, band, alb in (("flx_absdv", fd, 0, "albsnd"), ("flx_absdn", fd, 1, "albsnd"),
                               ("flx_absiv", fi, 0, "albsni"), ("flx_absin", fi, 1, "albsni")):
        exp = f[:, :, band] * (1.0 - B[alb][:, band : band + 1])
        assert np.array_equal(A[name][day], exp[day]), name
    snow = day & (A["h2osno"] > 0)
    assert snow.sum() > 100 and (A["albsnd"][snow] > 0).all()
    # all layer counts went through the solver
    assert set(np.unique(A["snl"][snow])) == {0, 1, 2, 3, 4, 5}


def test_soil_moist_stress_bit_exact_vs_reference():
    ft = H.field_table_from_oracle()
    cols, scal, soil = synth.make_state(ft, N, tier="B", seed=5)
    A = H.oracle_state(cols, scal, soil)
    A["frac_veg_nosno"][:] = 1
    # states the later kernels need
    A.frac_wet(); A.albedo_snicar(); A.canopy_hydrology(1800.0); A.surface_radiation(); A.canopy_temperature()
    B = A.clone()
    A.canopy_fluxes(1800.0)
    O.Reference().soil_moist_stress(B)
    for k in ("eff_porosity", "rootr"):
        assert np.array_equal(A[k], B[k]), k
    # btran is only the initial sum here (soybean adjustment never applies for vtype 12/14)
    assert np.array_equal(A["btran"], B["btran"])
    assert (A["btran"] > 0).any() and (A["btran"] == 0).any()


def test_scalar_helpers_bit_exact_vs_reference():
    import ctypes

    rng = np.random.default_rng(3)
    n = 20000
    R = O.Reference()
    L = O.lib().lib
    T = rng.uniform(180.0, 390.0, n)  # beyond both clamps of qsat
    p = rng.uniform(5.0e4, 1.05e5, n)
    ref = R.qsat(T, p)
    L.elmo_qsat.argtypes = [ctypes.c_double] * 2 + [ctypes.POINTER(ctypes.c_double)] * 4
    out = np.zeros((n, 4))
    o = [ctypes.c_double() for _ in range(4)]
    for i in range(n):
        L.elmo_qsat(T[i], p[i], *[ctypes.byref(x) for x in o])
        out[i] = [x.value for x in o]
    for k in range(4):
        assert np.array_equal(out[:, k], ref[k])
    q = rng.uniform(1e-4, 2e-2, n)
    rho, po2, pco2 = R.forc_derived(p, q, T)
    for name, refv, args in (("elmo_derive_forc_rho", rho, (p, q, T)), ("elmo_derive_forc_po2", po2, (p,)),
                             ("elmo_derive_forc_pco2", pco2, (p,))):
        f = getattr(L, name)
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_double] * len(args)
        got = np.array([f(*[a[i] for a in args]) for i in range(n)])
        assert np.array_equal(got, refv), name


def test_friction_velocity_bit_exact_vs_reference():
    import ctypes

    rng = np.random.default_rng(11)
    n = 20000
    kw = dict(
        ur=rng.uniform(1.0, 15.0, n), thv=rng.uniform(250.0, 310.0, n), dthv=rng.uniform(-8.0, 8.0, n),
        zldis=rng.uniform(2.0, 40.0, n), z0m=rng.uniform(0.001, 0.5, n), hgt_u=rng.uniform(10.0, 40.0, n),
        displa=rng.uniform(0.0, 3.0, n),
    )
    kw["z0h"] = kw["z0m"] * np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.1, 1.0, n))
    kw["z0q"] = np.where(rng.random(n) < 0.5, kw["z0h"], kw["z0h"] * 0.7)
    kw["hgt_t"] = kw["hgt_u"]
    kw["hgt_q"] = np.where(rng.random(n) < 0.5, kw["hgt_u"], kw["hgt_u"] + 1.0)
    ref = O.Reference().friction(**kw)
    L = O.lib().lib
    D = ctypes.c_double
    P = ctypes.POINTER(D)
    L.elmo_fv_monin_obukhov_length.argtypes = [D] * 5 + [P, P]
    L.elmo_fv_wind.argtypes = [D] * 5 + [P]
    L.elmo_fv_temp.argtypes = [D] * 4 + [P]
    L.elmo_fv_humidity.argtypes = [D] * 7 + [P]
    L.elmo_fv_temp2m.argtypes = [D] * 2 + [P]
    L.elmo_fv_humidity2m.argtypes = [D] * 4 + [P]
    got = np.zeros((n, 7))
    v = [D() for _ in range(7)]
    b = [ctypes.byref(x) for x in v]
    for i in range(n):
        k = {a: float(x[i]) for a, x in kw.items()}
        L.elmo_fv_monin_obukhov_length(k["ur"], k["thv"], k["dthv"], k["zldis"], k["z0m"], b[0], b[1])
        L.elmo_fv_wind(k["hgt_u"], k["displa"], v[0].value, v[1].value, k["z0m"], b[2])
        L.elmo_fv_temp(k["hgt_t"], k["displa"], v[1].value, k["z0h"], b[3])
        L.elmo_fv_humidity(k["hgt_q"], k["hgt_t"], k["displa"], v[1].value, k["z0h"], k["z0q"], v[3].value, b[4])
        L.elmo_fv_temp2m(v[1].value, k["z0h"], b[5])
        L.elmo_fv_humidity2m(v[1].value, k["z0h"], k["z0q"], v[5].value, b[6])
        got[i] = [x.value for x in v]
    assert np.array_equal(got, ref)
    # every branch of the profile functions was taken (zeta < -zetat, < 0, <= 1, > 1)
    zeta = (kw["hgt_t"] - kw["displa"]) / ref[:, 1]
    assert (zeta < -0.465).any() and ((zeta < 0) & (zeta >= -0.465)).any() and ((zeta >= 0) & (zeta <= 1)).any() and (zeta > 1).any()


# ---- next row: soil / snow temperature (soil_temperature_kokkos.cc).  The reference headers that build without
# Kokkos - soil_thermal_properties.h, pentadiagonal_solver.h, phase_change.h - against their restatements.
@pytest.fixture(scope="module")
def soil_states():
    ft = H.field_table_from_oracle()
    cols, scal, soil = synth.make_state(ft, 6000, tier="B", seed=77)
    S = H.oracle_state(cols, scal, soil)
    S.timestep7(1800.0)  # realistic fluxes / radiation for the surface heat flux terms
    return S


def test_soil_thermal_properties_bitwise(soil_states):
    S = soil_states
    got = S.soil_thermal()
    ref = S.soil_thermal(lib=O.Reference().R)
    for name, a, b in zip(("thk", "tk", "cv", "tk_h2osfc/c_h2osfc/dz_h2osfc"), got, ref):
        assert np.array_equal(a, b, equal_nan=True), name
    assert (got[0][:, 5:] > 0).all() and (got[2][:, 5:] > 0).all()
    snow = np.arange(5)[None, :] >= 5 - S["snl"][:, None]
    assert (got[0][:, :5][snow] > 0).all() and (got[0][:, :5][~snow] == 0).all()


def test_pentadiagonal_solver_bitwise(soil_states):
    S = soil_states.clone()
    ex = S.soil_temperature_ex(1800.0)
    a = O.pdma(soil_states["snl"], ex["lhs"], ex["rhs"])
    b = O.pdma(soil_states["snl"], ex["lhs"], ex["rhs"], lib=O.Reference().R)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a, ex["sol"], equal_nan=True)
    assert set(np.unique(soil_states["snl"])) == {0, 1, 2, 3, 4, 5}  # every system size 16..21 was solved


def test_phase_change_bitwise(soil_states):
    S = soil_states
    base = S.clone()
    ex = base.soil_temperature_ex(1800.0)  # leaves the matrix factor `fact` in the state
    c_h2osfc = S.soil_thermal()[3][:, 1]

    def prepared():
        rng = np.random.default_rng(9)
        T = S.clone()
        T["fact"][...] = base["fact"]
        T["t_soisno"][...] = np.where(S["t_soisno"] > 0, S["t_soisno"] + rng.uniform(-3, 3, S["t_soisno"].shape), 0)
        T["t_h2osfc"][...] = S["t_h2osfc"] + rng.uniform(-4, 2, S.ncols)
        return T

    A, B = prepared(), prepared()
    A.phase_change(1800.0, ex["hs"][:, 3], c_h2osfc)
    B.phase_change(1800.0, ex["hs"][:, 3], c_h2osfc, lib=O.Reference().R)
    assert not H.oracle_diffs(A, B)
    im = np.bincount(A["imelt"].ravel(), minlength=3)
    assert im[1] > 1000 and im[2] > 1000 and (A["qflx_h2osfc_ice"] != 0).sum() > 100  # melting, freezing, pond freezing
    assert (A["qflx_snomelt"] > 0).any() and (A["qflx_snofrz"] > 0).any()


# ---- rank 2 of the next rows: surface fluxes after the temperature solve, and the conservation diagnostics
def test_surface_fluxes_and_conservation_bitwise(soil_states):
    A = soil_states.clone()
    A.soil_temperature(1800.0)
    B = A.clone()
    A.surface_fluxes(1800.0)
    B.surface_fluxes(1800.0, lib=O.Reference().R)
    assert not H.oracle_diffs(A, B)
    da = A.evaluate_conservation(1800.0)
    db = B.evaluate_conservation(1800.0, lib=O.Reference().R)
    assert np.array_equal(da, db, equal_nan=True)
    # the branches: evaporation limited by the top layer's water, dew on snow / on ground, sublimation, capped snow
    assert (A["qflx_dew_snow"] > 0).any() and (A["qflx_dew_grnd"] > 0).any() and (A["qflx_sub_snow"] > 0).any()
    assert (A["qflx_evap_grnd"] > 0).any() and np.isfinite(da[:, [0, 1, 3, 4, 5, 7]]).all()
    # shortwave and longwave closures hold to rounding for every column (the physics upstream is consistent)
    assert np.abs(da[:, 4]).max() < 1e-9 and np.abs(da[:, 5]).max() < 1e-9


def test_init_timestep_column_kernel_bitwise(states):
    A, B = states[0].clone(), states[0].clone()
    A.init_timestep()
    B.init_timestep(lib=O.Reference().R)
    assert not H.oracle_diffs(A, B)
    assert np.array_equal(A["h2osno_old"], A["h2osno"]) and (A["do_capsnow"] == (A["h2osno"] > 1000.0)).all()


def test_get_forcing_and_phenology_bitwise(states):
    """kokkos_init_timestep's per-column functors ahead of its own kernel: the eight ComputeAtmForcing_* functors
    (atm_physics_impl.hh) in get_forcing's order, specific- and relative-humidity streams, and ComputePhenology, against
    the reference's own headers: every state field bit for bit.  The synthetic records sit on both sides of every clamp."""
    R = O.Reference().R
    if not hasattr(R, "elmref_get_forcing"):
        pytest.skip("oracle/_ref predates the forcing harness")
    rng = np.random.default_rng(5)
    for rh in (False, True):
        A, B = states[0].clone(), states[0].clone()
        if rh:
            for X in (A, B):
                X["atm_qbot"][...] = np.clip(X["atm_qbot"] * 4000.0, 0.0, 100.0)  # per cent
        e = rng.random(8)
        A.get_forcing(1.0 - e, e, rh)
        B.get_forcing(1.0 - e, e, rh, lib=R)
        assert not H.oracle_diffs(A, B)
        assert (A["forc_tbot"] == 323.0).any() and (A["forc_pbot"] == 4.0e4).any() and (A["forc_hgt_u_patch"] == 30.0).all()
        assert (A["forc_lwrad"] == 700.0).sum() == 0 and np.isfinite(A["forc_lwrad"]).all() and (A["forc_solad"] >= 0).all()
        assert (A["forc_rain"] >= 0).all() and (A["forc_snow"] >= 0).all() and ((A["forc_rain"] > 0) & (A["forc_snow"] > 0)).any()
    A, B = states[0].clone(), states[0].clone()
    for X in (A, B):
        X["vtype"][::7] = 0   # bare
        X["vtype"][1::7] = 14  # taller than the shrub limit: the 0.2 m burial rule
    A.phenology(0.3, 0.7)
    B.phenology(0.3, 0.7, lib=R)
    assert not H.oracle_diffs(A, B)
    assert (A["frac_veg_nosno_alb"] == 0).any() and (A["frac_veg_nosno_alb"] == 1).any() and (A["elai"] == 0).any()


def test_initialize_state_bitwise():
    """The per-column init functions of ELM::initialize_kokkos_elm (initialize_elm_kokkos.cc:373-428: topography, the initial
    snow mesh, soil hydraulic / thermal parameters, root fractions, initial temperature and water) - the producer of the
    state the hot path consumes.  All four reference headers compile here: the restatement (oracle/elmo_physics_h.c) equals
    the reference bit for bit, on every land unit, every snow-depth bin (edges included), mineral to pure organic soil."""
    R = O.Reference().R
    if not hasattr(R, "elmref_initialize_state"):
        pytest.skip("reference library predates elmref_initialize_state")
    pft, _ = synth.load_params()
    ft = H.field_table_from_oracle()
    lands = [dict(ltype=1, ctype=0, urbpoi=0, lakpoi=0), dict(ltype=2, ctype=0, urbpoi=0, lakpoi=0),
             dict(ltype=3, ctype=0, urbpoi=0, lakpoi=0), dict(ltype=4, ctype=0, urbpoi=0, lakpoi=0),
             dict(ltype=6, ctype=0, urbpoi=0, lakpoi=0), dict(ltype=5, ctype=0, urbpoi=0, lakpoi=1),
             dict(ltype=7, ctype=71, urbpoi=1, lakpoi=0), dict(ltype=7, ctype=73, urbpoi=1, lakpoi=0),
             dict(ltype=7, ctype=74, urbpoi=1, lakpoi=0), dict(ltype=7, ctype=75, urbpoi=1, lakpoi=0)]
    seen_snl = set()
    for k, land in enumerate(lands):
        cols, scal, soil = synth.make_state(ft, N, tier="B", seed=300 + k)
        cols["snow_depth"] = synth.init_snow_depths(N, 300 + k)
        vt = cols["vtype"].copy()
        vt[::9] = 0  # PFT::noveg: the zero-root branch
        cols["vtype"] = vt
        A = H.oracle_state(cols, scal, soil, dict(land, vtype=2))
        A.set_init_params(synth.ORGANIC_MAX, pft["roota_par"], pft["rootb_par"])
        B = A.clone()
        A.initialize_state()
        B.initialize_state(lib=R)
        assert H.oracle_diffs(A, B) == {}, land
        seen_snl |= set(np.unique(A["snl"]).tolist())
        assert np.isfinite(A["watsat"]).all() and (A["watsat"] > 0).all() and (A["watsat"] < 1).all()
    assert seen_snl == {0, 1, 2, 3, 4, 5}


# ---- kokkos_soil_temperature as a whole, by the reference's own per-column functions (oracle/ref_harness_soil.cc): surface
# heat fluxes, diffusive fluxes, matrix factor, the right-hand side and the banded matrix (soil_temp::detail::get_rhs_* /
# get_matrix_* / assemble_*), solve, temperature update, phase change, ground temperature.
@pytest.mark.skipif(O.lib().ref_soil is None, reason="oracle/_ref/libelmref_soil.so not built here")
def test_soil_temperature_whole_wrapper_bitwise(soil_states):
    for trial, mutate in enumerate((None, "pond", "warm")):
        A = soil_states.clone()
        if mutate == "pond":  # standing water on half of the columns, some of it about to freeze
            rng = np.random.default_rng(3)
            wet = rng.random(A.ncols) < 0.5
            A["h2osfc"][wet] = rng.uniform(1e-6, 8.0, wet.sum())
            A["frac_h2osfc"][wet] = rng.uniform(0.02, 0.6, wet.sum())
            A["t_h2osfc"][wet] = rng.uniform(270.0, 277.0, wet.sum())
        if mutate == "warm":  # melting packs
            A["t_soisno"][...] = np.where(A["t_soisno"] > 0, A["t_soisno"] + 4.0, 0.0)
            A["sabg_lyr"][...] *= 3.0
        B = A.clone()
        ea = A.soil_temperature_ex(1800.0)
        eb = B.soil_temperature_ref(1800.0)
        for k in ("hs", "rhs", "lhs"):
            assert np.array_equal(ea[k], eb[k], equal_nan=True), (trial, k)
        assert not H.oracle_diffs(A, B), trial
        # a second solve from the state the first one left (chained, as ELMInterface::advance does)
        A.soil_temperature(1800.0)
        B.soil_temperature_ref(1800.0)
        assert not H.oracle_diffs(A, B), trial
        assert set(np.unique(A["snl"])) == {0, 1, 2, 3, 4, 5}
        im = np.bincount(A["imelt"].ravel(), minlength=3)
        assert im[1] > 100 and im[2] > 100
    assert (soil_states["frac_h2osfc"] > 0).any() and (soil_states["frac_h2osfc"] == 0).any()


# ---- kokkos_snow_hydrology, one wrapper stage at a time, by the reference's own functions (oracle/ref_harness_snow.cc:
# snow_water, aerosol_phase_change, transpiration, snow_compaction, combine_layers, divide_layers, prune_snow_layers, snow_aging
# with the reference's own SnwRdsTable).  Columns in which the reference reads outside an array (the restatement raises a
# warning bit exactly there) are left out: its result there is whatever lies next to the array.  Not run by the reference: the
# two whole-array aerosol functions (their only body is a lambda for the Kokkos dispatch): those two stay "parity unpinned".
AERO = ("bcphi", "bcpho", "dst1", "dst2", "dst3", "dst4")


def _aerosol_inputs(S):
    return dict(snl=S["snl"].copy(), cap=S["do_capsnow"].copy(), q=S["qflx_snwcp_ice"].copy(), ice=S["h2osoi_ice"][:, :5].copy(),
                liq=S["h2osoi_liq"][:, :5].copy(), mss={a: S["mss_" + a].copy() for a in AERO})


def _check_aerosol_mass_and_concen(S, a, dt, what):
    """update_aerosol_mass_and_concen (aerosol_physics_impl.hh:67-106) is a whole-array function whose body is a lambda handed to
    the Kokkos-only dispatch: it cannot be instantiated here.  Its arithmetic, though, is two scalar helpers - get_snow_mass and
    get_snowcap_scl_fct (:10-31), which DO compile (ref_harness_snow.cc) - and, per layer and species, `mss *= scl; cnc = mss *
    (1.0 / snowmass)` (:84-103).  The restatement's stage is pinned through them: the reference's own helper values, the two
    products formed here in IEEE double, every bit of the twelve arrays compared."""
    n = a["snl"].shape[0]
    sl = np.broadcast_to(np.arange(5, dtype=np.int32), (n, 5))
    top = np.broadcast_to((5 - a["snl"]).astype(np.int32)[:, None], (n, 5))
    cap = np.broadcast_to(a["cap"].astype(np.int32)[:, None], (n, 5))
    q = np.broadcast_to(a["q"][:, None], (n, 5))
    mass, scl = O.aerosol_helpers_ref(sl, top, cap, a["ice"], a["liq"], q, dt)
    inv = 1.0 / mass
    for sp in AERO:
        m = a["mss"][sp] * scl
        for name, exp in (("mss_" + sp, m), ("cnc_" + sp, m * inv)):
            got = S[name]
            eq = (got.view(np.uint64) == exp.view(np.uint64)) | (np.isnan(got) & np.isnan(exp))
            assert eq.all(), (what, name, int((~eq).sum()))
    return int((sl >= top).sum())


@pytest.mark.skipif(O.lib().ref_snow is None, reason="oracle/_ref/libelmref_snow.so not built here")
def test_snow_hydrology_stages_bitwise_vs_reference():
    DT = 1800.0
    ft = H.field_table_from_oracle()
    seen_snl_change = {5: 0, 6: 0}
    aged = 0
    pinned_aero = 0
    compared = {s: 0 for s in O.OracleState.SNOW_STAGES_REF}
    skipped = 0
    for seed in (5, 21):
        cols, scal, soil = synth.make_state(ft, 6016, tier="B", seed=seed)
        S = H.oracle_state(cols, scal, soil)  # (the snow-aging tables are set by the helper)
        for step in range(4):  # chained model steps: packs are built by snowfall, compacted, split, merged and pruned
            S.init_timestep()
            S.timestep7(DT)
            S.soil_temperature(DT)
            for stage in range(len(S.SNOW_STAGES)):
                ref_runs = stage in S.SNOW_STAGES_REF
                R = S.clone() if ref_runs else None
                before = S["err_flags"].copy()
                snl_before = S["snl"].copy()
                R0_rds = S["snw_rds"].copy()
                aero_in = _aerosol_inputs(S) if stage == 8 else None
                S.snow_hydrology_stage(DT, stage)
                if stage == 8:
                    pinned_aero += _check_aerosol_mass_and_concen(S, aero_in, DT, (seed, step))
                if not ref_runs:
                    continue
                raised = S["err_flags"] & ~before
                skip = (raised & (H.WARN_WATER | H.WARN_COMBINE)) != 0
                R["err_flags"][...] = 0
                threw = R.snow_hydrology_stage(DT, stage, ref=True, skip=skip)
                ref_threw = (R["err_flags"] >> 31) != 0
                # the reference throws exactly where the restatement raises the divide_layers radius flag / snow_aging's dr_fresh flag
                assert threw == int(ref_threw.sum()) and np.array_equal(ref_threw, (raised & (H.ERR_DIVIDE | H.ERR_AGE)) != 0), (seed, step, stage)
                ok = ~skip & ~ref_threw
                for k in S.fields:
                    if k == "err_flags":
                        continue
                    a, b = S.fields[k][ok], R.fields[k][ok]
                    eq = (a == b) | (np.isnan(a.astype(float)) & np.isnan(b.astype(float)))
                    assert eq.all(), (seed, step, S.SNOW_STAGES[stage], k, int((~eq).sum()))
                compared[stage] += int(ok.sum())
                skipped += int(skip.sum())
                if stage in seen_snl_change:
                    seen_snl_change[stage] += int((S["snl"] != snl_before).sum())
                if stage == 9:
                    aged += int((S["snw_rds"] != R0_rds).any(axis=1).sum())
            S.surface_fluxes(DT)
    # the comparison saw what it is meant to see: layers merged and split, and only a small share of columns was left out
    assert seen_snl_change[5] > 200 and seen_snl_change[6] > 200, seen_snl_change
    assert pinned_aero > 50000, pinned_aero  # layers inside a pack whose aerosol masses / concentrations were pinned (stage 8)
    assert aged > 8000, aged  # snow_aging grew the grains of the layered packs (table look-ups included)
    assert min(compared.values()) > 40000 and skipped < 0.15 * compared[0], (compared, skipped)  # (five-layer packs: 10 % of tier B)
