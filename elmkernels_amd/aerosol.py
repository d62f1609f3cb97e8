"""Aerosol deposition from a monthly climatology, on the host (include/elmk.h "aerosol deposition"; ELM's aerdepini / aerinterp), in
numpy only: the restatement of what k_aerosol_deposition computes, in its operation order, and a synthetic climatology.

    series = aerosol.synthetic_climatology(ncells)            # {stream: [12, ncells]}
    idx, w = regrid.nearest_map(lat, lon, nlon, nlat)         # the reference's nearest-cell pick (or regrid.bilinear_map)
    S.aerosol_reserve(ncells, idx, w)
    for name in aerosol.STREAMS:
        S.aerosol_upload(name, 0, series[name])
    S.run(dt, steps, st.RUN_AEROSOL)                          # every step: aer_* from the step's month bracket
    want = aerosol.interpolate(series, m1, m2, wt1, wt2, idx, w)   # what one elmk_aerosol_deposition writes, bit for bit

For every stream s and column c, every line one IEEE fp64 operation:
    r1 = apply_map(idx, w, series[s][m1]);  r2 = apply_map(idx, w, series[s][m2])      (no map: the month's values themselves)
    aer_s = wt1 * r1 + wt2 * r2
Both products are formed whatever the weights: (1, 0) gives x * 1 + y * 0, not a copy of x, so a NaN or infinity in the other month
propagates and a -0.0 in month m1 becomes +0.0 once 0 * y = +0.0 is added.
"""
import numpy as np

from . import regrid

# member order of aero_data::AerosolFileInput (src/data/aerosol_data.h:11-22) = field order aer_bcphi .. aer_dst4_2
STREAMS = ("bcphi", "bcpho", "bcdep", "dst1_1", "dst1_2", "dst2_1", "dst2_2", "dst3_1", "dst3_2", "dst4_1", "dst4_2")
FIELDS = tuple("aer_" + s for s in STREAMS)
NMONTHS = 12
RUN_AEROSOL = 8  # ELMK_RUN_AEROSOL


def _series_of(series, s):
    if isinstance(series, dict):
        a = series[s] if s in series else series["aer_" + s]
    else:
        a = np.asarray(series)[STREAMS.index(s)]
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != NMONTHS:
        raise ValueError(f"{s}: the series must be [12, ncells]")
    return a


def interpolate(series, m1, m2, wt1, wt2, idx=None, w=None):
    """The eleven aer_* fields one elmk_aerosol_deposition(m1, m2, wt1, wt2) writes: series is {stream: [12, ncells]} (keys as
    STREAMS or FIELDS) or an array [11, 12, ncells]; idx / w the ELL map of elmk_aerosol_reserve ([npts, ncols], -1 = padding), or
    both None for per-column series.  Returns {stream: float64 [ncols]} in fp64 (the fp32-state build rounds on store:
    .astype(np.float32))."""
    m1, m2 = int(m1), int(m2)
    if not (0 <= m1 < NMONTHS and 0 <= m2 < NMONTHS):
        raise ValueError("months are 0 .. 11")
    if (idx is None) != (w is None):
        raise ValueError("idx and w: both or neither")
    wt1, wt2 = np.float64(wt1), np.float64(wt2)
    out = {}
    with np.errstate(all="ignore"):
        for s in STREAMS:
            a = _series_of(series, s)
            r1 = a[m1] if idx is None else regrid.apply_map(idx, w, a[m1])
            r2 = a[m2] if idx is None else regrid.apply_map(idx, w, a[m2])
            t1 = wt1 * r1
            t2 = wt2 * r2
            out[s] = t1 + t2
    return out


def month_bracket(doy_fraction, days_in_year=365.0):
    """(m1, m2, wt1, wt2) of a time of year in days since 1 January 00:00 by mid-month interpolation on equal months - enough for
    demos and tests; a driver uses its calendar's (monthly_data.cc:29-62), the same call that feeds elmk_phenology."""
    x = (float(doy_fraction) % days_in_year) / days_in_year * NMONTHS - 0.5
    m1 = int(np.floor(x)) % NMONTHS
    wt2 = x - np.floor(x)
    return m1, (m1 + 1) % NMONTHS, 1.0 - wt2, wt2


def synthetic_climatology(ncells, seed=0):
    """A seasonal climatology {stream: [12, ncells]} in kg/m2/s for tests and demos: black carbon with a weak winter maximum, dust
    (dst1 .. dst4, dry _1 and wet _2) peaking in spring (April), every stream with its own amplitude and a cell pattern of its own.
    Edge values on purpose: cells 1 and ncells - 2 (where they exist) are exactly zero in every stream and month (ocean far from any
    source), and cell 0 of dst1_1 is -0.0 in January."""
    ncells = int(ncells)
    rng = np.random.default_rng(seed)
    mon = np.arange(NMONTHS, dtype=np.float64)
    spring = 0.5 * (1.0 + np.cos(2.0 * np.pi * (mon - 3.0) / 12.0))  # 1 in April, 0 in October
    winter = 0.5 * (1.0 + np.cos(2.0 * np.pi * mon / 12.0))  # 1 in January
    out = {}
    for k, s in enumerate(STREAMS):
        pattern = rng.random(ncells) ** 2  # most cells far from a source
        if s.startswith("bc"):
            amp, season = 2.0e-13 * (1.0 + 0.3 * k), 0.7 + 0.3 * winter
        else:
            amp, season = 5.0e-11 * (1.0 + 0.2 * k), 0.05 + 0.95 * spring**2
        a = amp * season[:, None] * pattern[None, :]
        for c in (1, ncells - 2):
            if 0 <= c < ncells:
                a[:, c] = 0.0
        out[s] = a
    if ncells > 0:
        out["dst1_1"][0, 0] = -0.0
    return out
