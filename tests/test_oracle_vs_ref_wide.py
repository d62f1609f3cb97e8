"""The oracle against the reference's own code (oracle/_ref) on tier W (synth.wide_mix): inputs over their physical range and
the edge rows of the paths the fixture-near tiers never reach.  This pins the oracle on those branches before the device is
judged against it there (tests/test_gpu_wide.py).  Bar: bit for bit, as in tests/test_oracle_vs_ref.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import helpers as H
from tests import parity_cases as P

pytestmark = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref/libelmref.so not built here")

DT = P.DT
NOFLAGS = lambda S: [k for k in S.fields if k != "err_flags"]  # noqa: E731


def _wide(name, land=None):
    case = P.BY_NAME[name]
    cols, scal, soil = P.state(case, H.field_table_from_oracle())
    return H.oracle_state(cols, scal, soil, land or case.land)


@pytest.mark.parametrize("name", ["W_wrappers", "W_oldfflag", "W_dewmx"])
def test_five_wrappers_bit_exact_on_wide_inputs(name):
    A = _wide(name)
    B = A.clone()
    R = O.Reference()
    A.frac_wet(); R.frac_wet(B)
    assert not H.oracle_diffs(A, B, NOFLAGS(A))
    A.canopy_hydrology(DT); R.canopy_hydrology(B, DT)
    assert not H.oracle_diffs(A, B, NOFLAGS(A))
    A.albedo_snicar()
    for k in A.fields:
        B.fields[k][...] = A.fields[k]
    for a, r in ((A.surface_radiation, R.surface_radiation), (A.canopy_temperature, R.canopy_temperature),
                 (A.bareground_fluxes, R.bareground_fluxes)):
        a(); r(B)
        d = H.oracle_diffs(A, B, NOFLAGS(A))
        assert not d, d
    assert not (A["err_flags"] & 0x7FF).any()


def test_snicar_bit_exact_on_wide_inputs():
    A = _wide("W_wrappers")
    A.albedo_snicar()
    B = A.clone()
    B["albsnd"][:] = -1.0
    B["albsni"][:] = -1.0
    O.Reference().snicar(B)
    assert not (B["err_flags"] & H.REF_THREW).any() and not (A["err_flags"] & 0x7FF).any()
    assert np.array_equal(A["albsnd"], B["albsnd"]) and np.array_equal(A["albsni"], B["albsni"])
    snow = (A["coszen"] > 0) & (A["h2osno"] > 0)
    assert set(np.unique(A["snl"][snow])) == {0, 1, 2, 3, 4, 5}


@pytest.mark.skipif(O.lib().ref_canopy is None, reason="oracle/_ref/libelmref_canopy.so not built here")
@pytest.mark.parametrize("name", ["W_wrappers", "W_short_day", "W_abi_default"])
def test_canopy_fluxes_bit_exact_on_wide_inputs(name):
    A = _wide(name)
    for step in range(2):
        A.frac_wet(); A.albedo_snicar(); A.canopy_hydrology(DT); A.surface_radiation(); A.canopy_temperature()
        A.bareground_fluxes()
        B = A.clone()
        O.psn_counters(reset=True)
        A.canopy_fluxes(DT)
        counts = O.psn_counters()
        B.canopy_fluxes_ref(DT)
        assert not (B["err_flags"] & H.REF_THREW).any() and not (A["err_flags"] & 0x7FF).any()
        d = H.oracle_diffs(A, B, NOFLAGS(A))
        assert not d, (step, d)
    assert counts["brent"] > 0 and counts["c4"] > 0, counts


@pytest.mark.skipif(O.lib().ref_soil is None, reason="oracle/_ref/libelmref_soil.so not built here")
@pytest.mark.parametrize("name", ["W_advance", "W_oldfflag"])
def test_soil_temperature_and_surface_fluxes_bit_exact_on_wide_inputs(name):
    A = _wide(name)
    A.init_timestep()
    A.timestep7(DT)
    B = A.clone()
    A.soil_temperature(DT)
    B.soil_temperature_ref(DT)
    d = H.oracle_diffs(A, B, NOFLAGS(A))
    assert not d, d
    im = np.bincount(A["imelt"].ravel(), minlength=3)
    assert im[1] > 0 and im[2] > 0 and (A["qflx_h2osfc_ice"] != 0).any()
    top = (np.arange(A.ncols), 5 - A["snl"])
    egsmax = np.maximum(A["h2osoi_ice"][top] + A["h2osoi_liq"][top], 0.0) / DT
    limited = A["qflx_evap_soi"] > 2.0 * egsmax  # evaporation far beyond what the top layer holds: the egirat < 1 path
    B = A.clone()
    A.surface_fluxes(DT)
    B.surface_fluxes(DT, lib=O.Reference().R)
    assert not H.oracle_diffs(A, B)
    assert np.array_equal(A.evaluate_conservation(DT), B.evaluate_conservation(DT, lib=O.Reference().R), equal_nan=True)
    assert limited.any()


@pytest.mark.skipif(O.lib().ref_snow is None, reason="oracle/_ref/libelmref_snow.so not built here")
def test_snow_hydrology_stages_bit_exact_on_wide_inputs():
    S = _wide("W_advance")
    merged = 0
    for step in range(3):
        S.init_timestep()
        S.timestep7(DT)
        S.soil_temperature(DT)
        for stage in range(len(S.SNOW_STAGES)):
            before = S["err_flags"].copy()
            snl_before = S["snl"].copy()
            R = S.clone() if stage in S.SNOW_STAGES_REF else None
            S.snow_hydrology_stage(DT, stage)
            if R is None:
                continue
            raised = S["err_flags"] & ~before
            skip = (raised & (H.WARN_WATER | H.WARN_COMBINE)) != 0
            R["err_flags"][...] = 0
            R.snow_hydrology_stage(DT, stage, ref=True, skip=skip)
            ref_threw = (R["err_flags"] >> 31) != 0
            assert np.array_equal(ref_threw, (raised & (H.ERR_DIVIDE | H.ERR_AGE)) != 0), (step, stage)
            ok = ~skip & ~ref_threw
            for k in NOFLAGS(S):
                a, b = S.fields[k][ok], R.fields[k][ok]
                eq = (a == b) | (np.isnan(a.astype(float)) & np.isnan(b.astype(float)))
                assert eq.all(), (step, S.SNOW_STAGES[stage], k, int((~eq).sum()))
            if stage == 5:
                merged += int((S["snl"] < snl_before).sum())
        S.surface_fluxes(DT)
    assert merged > 20, merged
