"""HIP kernels against the oracle on tier W (tests/parity_cases.py: wide inputs, edge rows, the context-scalar variants and
the land units).  Bar: every field and err_flags bit for bit, as in tests/test_gpu_parity.py."""
import numpy as np
import pytest

from elmkernels_amd import state as st
from tests import helpers as H
from tests import parity_cases as P
from tests import run_cases as GR

pytestmark = pytest.mark.gpu

DT = P.DT


def _pair(case, n=None, set_scalars=True):
    cols, scal, soil = P.state(case if n is None else P.Case(case.name, case.tier, n, case.seed, scalars=case.scalars),
                               st.field_table())
    S = H.oracle_state(cols, scal, soil, case.land)
    # (scal None: a context that never calls elmk_set_scalars runs on the library's defaults, parity_cases.ABI_DEFAULT)
    return H.device_state(cols, scal if set_scalars else None, soil, case.land), S


def _check(D, S, what):
    assert np.array_equal(D["err_flags"], S["err_flags"]), f"{what}: err_flags differ"
    worst, bad = H.compare_states(D, S, bitwise=True)
    assert not bad, f"{what}: worst rel err {worst:.3e}; not bit-identical: {bad}"


def _resync(D, S):
    for k, v in S.fields.items():
        if k != "err_flags":
            D[k] = v


@pytest.mark.parametrize("name", ["W_wrappers", "W_oldfflag", "W_dewmx", "W_short_day"])
def test_each_wrapper_on_wide_inputs(name):
    D, S = _pair(P.BY_NAME[name])
    calls = [
        ("frac_wet", lambda: st.kokkos_frac_wet(D), S.frac_wet),
        ("albedo_snicar", lambda: st.kokkos_albedo_snicar(D), S.albedo_snicar),
        ("canopy_hydrology", lambda: st.kokkos_canopy_hydrology(D, DT), lambda: S.canopy_hydrology(DT)),
        ("surface_radiation", lambda: st.kokkos_surface_radiation(D), S.surface_radiation),
        ("canopy_temperature", lambda: st.kokkos_canopy_temperature(D), S.canopy_temperature),
        ("bareground_fluxes", lambda: st.kokkos_bareground_fluxes(D), S.bareground_fluxes),
        ("canopy_fluxes", lambda: st.kokkos_canopy_fluxes(D, DT), lambda: S.canopy_fluxes(DT)),
        ("soil_temperature", lambda: st.kokkos_soil_temperature(D, DT), lambda: S.soil_temperature(DT)),
        ("snow_hydrology", lambda: st.kokkos_snow_hydrology(D, DT), lambda: S.snow_hydrology(DT)),
        ("surface_fluxes", lambda: st.kokkos_surface_fluxes(D, DT), lambda: S.surface_fluxes(DT)),
    ]
    for what, dev, ora in calls:
        dev()
        ora()
        _check(D, S, f"{name}/{what}")
        _resync(D, S)
    D.close()


@pytest.mark.parametrize("name", ["W_wrappers", "W_dewmx", "W_short_day", "W_abi_default"])
def test_fused_and_plain_steps_on_wide_inputs(name):
    """elmk_timestep7 then elmk_timestep7_fused, chained with no re-synchronisation; W_abi_default runs on a context that
    never had its scalars set (the library's defaults, oldfflag = 1 and no day length)."""
    case = P.BY_NAME[name]
    D, S = _pair(case, set_scalars=name != "W_abi_default")
    for step in range(case.steps):
        (st.timestep7_fused if step % 2 else st.timestep7)(D, DT)
        S.timestep7(DT)
        _check(D, S, f"{name} step {step}")
    D.close()


@pytest.mark.parametrize("name", ["W_advance", "W_oldfflag"] + [f"W_land{k}" for k in range(9)])
def test_advance_chain_on_wide_inputs(name):
    """init_timestep, the seven (per wrapper, fused, or the single call elmk_advance_physics, plain and as a replayed HIP graph:
    step % 4 = 0, 1, 2, 3), soil_temperature, snow_hydrology, surface_fluxes chained with no re-synchronisation, the oracle
    driven by parity_cases.oracle_step (the chain the coverage test replays): every field bit-identical at every step, thin
    layers removed by combine_layers on the device as in the oracle, and the conservation diagnostics of the last step."""
    case = P.BY_NAME[name]
    assert case.steps >= 4  # every mode, the graph replay included, runs on every case
    D, S = _pair(case)
    hgt = P.heights(S)
    snl0 = S["snl"].copy()
    for step in range(case.steps):
        for k, v in hgt.items():
            D[k] = v
        st.kokkos_init_timestep(D)
        mode = step % 4
        if mode >= 2:
            D.set_graph(mode == 3)
            st.advance_physics(D, DT)
            D.set_graph(False)
        else:
            (st.timestep7_fused if mode else st.timestep7)(D, DT)
            st.kokkos_soil_temperature(D, DT)
            st.kokkos_snow_hydrology(D, DT)
            st.kokkos_surface_fluxes(D, DT)
        P.oracle_step(S, case, hgt)
        _check(D, S, f"{name} step {step}")
    mms, cols = st.kokkos_evaluate_conservation(D, DT, per_column=True)
    ref = S.evaluate_conservation(DT)
    ponded = S["frac_h2osfc"] != 0  # pow(t_h2osfc_bef, 40) there (reference quirk): held as test_surface_fluxes_and_conservation_diagnostics holds it
    same = (cols == ref) | (np.isnan(cols) & np.isnan(ref))  # (NaN where the land unit's canopy fluxes are NaN in both)
    e = np.where(same, 0.0, np.abs(cols - ref) / np.maximum(np.abs(ref), 1e-6))
    assert e[~ponded].max(initial=0.0) < 1e-12 and e[ponded][:, [0, 1, 2, 3, 4, 5, 7]].max(initial=0.0) < 1e-12
    assert (S["snl"] < snl0).sum() > 20  # packs lost layers (on the device too: snl is compared above)
    D.close()


@pytest.mark.parametrize("n", [1, 63, 65, 1001])
def test_ragged_sizes_on_wide_inputs(n):
    D, S = _pair(P.BY_NAME["W_wrappers"], n=n)
    for step in range(2):
        (st.timestep7_fused if step else st.timestep7)(D, DT)
        S.timestep7(DT)
        _check(D, S, f"W n={n} step {step}")
    D.close()


def test_large_launch_structure_on_wide_inputs():
    """262 144 wide columns (the base block and its edge rows tiled) through the fused step and the whole advance() call,
    every field bit-identical to the oracle.  The classes of the large launch structure are populated: the leaf-temperature
    iteration reaches its limit of 41 trips in many columns, the bare-ground list and every SNICAR layer-count class are
    filled (their lists are drained by the call that fills them, so the state is what shows they were used)."""
    n = 262_144
    D, S = _pair(P.BY_NAME["W_wrappers"], n=n)
    day_snow = (S["coszen"] > 0) & (S["h2osno"] > 0)
    assert all((day_snow & (S["snl"] == k)).sum() > 1000 for k in range(6))
    st.timestep7_fused(D, DT)
    S.timestep7(DT)
    _check(D, S, "W 262144 fused")
    assert (S["frac_veg_nosno"] == 0).sum() > 10000  # the bare-ground list
    trips = D.canopy_trip_counts()
    assert trips.max() == 41 and (trips == 41).sum() > 1000 and (trips == 0).any()
    st.advance_physics(D, DT)
    S.timestep7(DT)
    S.soil_temperature(DT)
    S.snow_hydrology(DT)
    S.surface_fluxes(DT)
    _check(D, S, "W 262144 advance_physics")
    D.close()


def test_hot_path_on_device_against_the_reference_library_on_wide_inputs():
    """HIP against the reference's own functions (oracle/_ref) with no restatement in between, on tier W and its short-day
    variant: three chained steps of the seven wrappers, every field bit for bit (as test_gpu_parity's tier-B test)."""
    from oracle import oracle as O
    from tests import _parity_mode

    if not (O.have_ref() and O.have_ref_canopy()):
        pytest.skip("oracle/_ref libraries not built")
    if not _parity_mode.BITWISE_VALID:
        pytest.skip("another host libm than the one the device math restates")
    R = O.Reference()
    for name in ("W_wrappers", "W_short_day"):
        D, B = _pair(P.BY_NAME[name])
        for step in range(3):
            (st.timestep7_fused if step == 1 else st.timestep7)(D, DT)
            R.frac_wet(B)
            B.albedo_snicar_ref()
            R.canopy_hydrology(B, DT)
            R.surface_radiation(B)
            R.canopy_temperature(B)
            R.bareground_fluxes(B)
            B.canopy_fluxes_ref(DT)
            assert not (B["err_flags"] >> 31).any(), "the reference threw"
            worst, bad = H.compare_states(D, B, bitwise=True)
            assert not bad, (name, step, bad)
        D.close()


def test_run_equals_stepwise_on_wide_inputs():
    """elmk_run (twelve steps replayed from one captured step) against the same steps called one by one, on tier W: state,
    err_flags, conservation and flag rows bit for bit (tests/run_cases.py's harness)."""
    base = GR._inputs(5003, 91, tier="W")  # (a ragged size: the harness wants a padded level stride)
    cols, _, _, _, _, rec = base
    A, B = GR._pair(base)
    steps = GR.schedule()
    want = GR.stepwise(A, rec, steps)
    B.run_reserve(GR.NREC, GR.NSTEPS)
    GR.upload_series(B, rec)
    B.run(DT, steps)
    GR.assert_same_rows(B.run_diagnostics(), want)
    GR.assert_same_state(A, B, cols)
    A.close()
    B.close()


def test_per_column_day_length_on_wide_inputs():
    """Per-column solar geometry and day length (set_column_geography) on tier W: two steps of the whole chain checked against
    the oracle run once per group of columns sharing (dayl, max_dayl), bit for bit (tests/run_cases.py's harness)."""
    n = 8192
    D, cols, scal, soil = GR._global_pair(n, 35, tier="W")
    oracles = {}
    for step, decday in enumerate((172.25, 172.3125)):
        D.solar_geometry(DT, decday, int(decday) - 1)
        coszen = D["coszen"].copy()
        dayl, max_dayl = D.day_length()
        groups = GR._groups(dayl, max_dayl)
        assert len(groups) >= 2
        GR._device_step(D, "advance")
        for dl, mdl, m in groups:
            key = (dl.tobytes(), mdl.tobytes())
            if key not in oracles:
                oracles[key] = H.oracle_state(cols, dict(scal, dayl=float(dl), max_dayl=float(mdl)), soil)
            GR._oracle_step(oracles[key], coszen)
            worst, bad = H.compare_states(D, oracles[key], skip_cols=~m, bitwise=True)
            assert not bad, (step, float(dl), float(mdl), bad)
    D.close()
