"""Shortwave COSZEN mode on the host (include/elmk.h "shortwave"): the numpy restatement of ELM's cos(zenith) factor on its edge
cases, and the property the energy claim rests on - the reference's own average_cosz (oracle/_ref) is additive over the steps of a
forcing interval, so the steps' factors cz / czf average to one over the interval."""
import ctypes as C
import math

import numpy as np
import pytest

from elmkernels_amd import coszen_factor, synth


def _scalar(cz, czf):
    """fac = (cz > 0.001) ? std::min(cz / czf, 10.0) : 0.0 in plain Python floats (IEEE division by zero as C does it)."""
    if not cz > 0.001:
        return 0.0
    if czf == 0.0:
        q = math.copysign(math.inf, cz) * math.copysign(1.0, czf)
    else:
        q = cz / czf
    return 10.0 if 10.0 < q else q  # std::min(q, 10.0): q wins ties and NaN


def test_coszen_factor_edge_cases():
    above = np.nextafter(0.001, 1.0)
    cz = np.array([0.0, 0.001, above, np.nan, 0.5, 0.5, 0.5, 0.05, 0.5, 1.0, -0.2, 0.3, 0.3, np.inf])
    czf = np.array([0.3, 0.3, 0.3, 0.3, 0.0, 0.05, 0.049, 0.005, np.nan, 0.1, 0.1, -0.0, 0.7, 0.2])
    got = coszen_factor(cz, czf)
    want = np.array([_scalar(a, b) for a, b in zip(cz.tolist(), czf.tolist())])
    same_bits = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert same_bits.all(), (got, want)
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == above / 0.3  # the threshold is strict
    assert got[3] == 0.0  # NaN cos(zenith): not above the threshold
    assert got[4] == 10.0 and got[5] == 10.0 and got[6] == 10.0  # czf = 0 and the tie at the cap
    assert got[7] == 10.0  # 0.05 / 0.005 rounds to 10 or just above: capped either way
    assert np.isnan(got[8])  # a NaN quotient wins min, as in std::min
    assert got[11] == -np.inf  # cz / -0.0 is -inf, below the cap
    assert got[13] == 10.0  # an infinite cos(zenith) is capped


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


# Where the interval's mean cos(zenith) czf is at least CZF_EXACT, the sum of the steps' means equals the interval's mean within
# 1e-12 relative.  Below it the sun is near the horizon for the whole interval: integrate_cosz's two terms, each of order one over
# dtrad, cancel, and both sides carry the same absolute rounding, measured at most 6e-14 in cos(zenith) here (1 h records) - so the
# relative claim is restricted to czf >= CZF_EXACT and the rest is bounded absolutely.  No branch of avg_hourangle breaks the sum:
# the residue follows czf, not the branch, and vanishes where the sun stays down (czf == 0 and every step 0).
CZF_EXACT = 0.1
ABS_BOUND = 1e-13


@pytest.mark.parametrize("forc_hours", [1, 3, 6, 24])
def test_reference_average_cosz_is_additive_over_an_interval(forc_hours):
    """4 096 columns over the globe, records aligned on the day, several days of the year, model steps of 30 and 15 minutes:
    sum_s average_cosz(dt, rec + s dt / 86400) dt == average_cosz(forc_dt, rec) forc_dt within 1e-12 relative (absolute floor 1e-15,
    in cos(zenith)) wherever czf >= CZF_EXACT, and within ABS_BOUND in cos(zenith) everywhere."""
    cosz = _ref_solar()
    n = 4096
    lat, lon = synth.global_grid(n, seed=404)
    forc_dt = forc_hours * 3600.0
    checked = 0
    for day in (0.0, 79.0, 171.0, 264.0, 354.0, 364.0):
        for k in range(24 // forc_hours):
            rec = day + 1.0 + k * forc_dt / 86400.0
            czf = cosz(lat, lon, forc_dt, rec)
            whole = czf * forc_dt
            for dt in (1800.0, 900.0):
                parts = np.zeros(n)
                for s in range(int(forc_dt // dt)):
                    parts += cosz(lat, lon, dt, rec + s * dt / 86400.0) * dt
                err = np.abs(parts - whole)
                exact = czf >= CZF_EXACT
                tol = 1e-12 * np.abs(whole) + 1e-15 * forc_dt
                assert (err[exact] <= tol[exact]).all(), (day, k, dt, float((err[exact] / whole[exact]).max()))
                assert (err <= ABS_BOUND * forc_dt).all(), (day, k, dt, float(err.max() / forc_dt))
                assert (err[czf == 0.0] == 0.0).all()
                checked += int(exact.sum())
    assert checked > n  # the claim covers most daylit intervals
