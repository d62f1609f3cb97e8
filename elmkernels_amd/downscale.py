"""Downscaling of coarse-grid forcing to column elevation on the host (include/elmk.h "downscaling"): ELM's downscale_forcings
restated in the device's operation order, so that the tests can compare the TOPO forcing kernels bit for bit.  numpy only.

exp is math.exp per element: glibc's exp is what the device's elmk_exp restates bit for bit, np.exp is not guaranteed to be.  qsat is
the caller's (the tests use oracle.qsat, pinned bit for bit to the reference's own): a function (T, p) -> qs over float64 arrays.  The group
sums go through regrid.apply_aggregate, the host statement of the device's aggregation.
"""
import math

import numpy as np

from . import regrid as RG

DS_OFF, DS_TOPO = 0, 1  # elmk_set_downscaling
DS_MODES = {"off": DS_OFF, "topo": DS_TOPO}
LAPSE, LAPSE_LW, LW_LIMIT = 0.006, 0.032, 0.5  # CLM5 / ELM namelist defaults: K/m, W m-2 per m, fraction
ZBOT = 30.0  # ProcessZBOT's forc_hgt

# src/data/elm_constants.h, formed by the same expressions as elmk_dev.h
TFRZ = 273.15
BOLTZ = 1.38065e-23
AVOGAD = 6.02214e26
RGAS = AVOGAD * BOLTZ
MWDAIR = 28.966
RAIR = RGAS / MWDAIR
GRAV = 9.80616
CPAIR = 1.00464e3


def _exp(x):
    x = np.asarray(x, dtype=np.float64)
    return np.array([math.exp(v) for v in x.reshape(-1)], dtype=np.float64).reshape(x.shape)


def _min(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return np.where(b < a, b, a)


def _max(a, b):
    """std::max(a, b) = (a < b) ? b : a"""
    return np.where(a < b, b, a)


def downscale(tg, pg, qg, lg, prec, hc, hf, qsat, lapse=LAPSE, lapse_lw=LAPSE_LW, lw_limit=LW_LIMIT):
    """The per-column contract of include/elmk.h "downscaling", elementwise over float64 arrays.

    tg, pg, qg, lg: tbot, pbot, qbot, lwrad as get_forcing computes them (the forcing's values at its surface height hf); prec: the
    PREC record (ProcessPREC clamps it at 0 first, as here); hc: the column's elevation.  Returns a dict of the fields the TOPO kernel
    writes: forc_tbot, forc_thbot, forc_pbot, forc_qbot, forc_lwrad (before any group renormalisation), forc_rain, forc_snow."""
    tg, pg, qg, lg, prec, hc, hf = (np.asarray(a, dtype=np.float64) for a in (tg, pg, qg, lg, prec, hc, hf))
    with np.errstate(all="ignore"):
        dz = hc - hf
        tc = tg - lapse * dz
        hbot = RAIR * 0.5 * (tg + tc) / GRAV
        pc = pg * _exp(-dz / hbot)
        thc = tg + (tc - tg) * _exp((ZBOT / hbot) * (RAIR / CPAIR))
        qs_g = np.asarray(qsat(tg, pg), dtype=np.float64)
        qs_c = np.asarray(qsat(tc, pc), dtype=np.float64)
        qc = qg * (qs_c / qs_g)
        lc = _max(_min(lg - lapse_lw * dz, lg * (1.0 + lw_limit)), lg * (1.0 - lw_limit))
        frac = _min(1.0, _max(0.0, (tc - TFRZ) * 0.5))
        p = _max(prec, 0.0)
        rain = frac * p
        snow = (1.0 - frac) * p
    return {"forc_tbot": tc, "forc_thbot": thc, "forc_pbot": pc, "forc_qbot": qc, "forc_lwrad": lc, "forc_rain": rain,
            "forc_snow": snow}


def check_groups(ptr, col, w, ncols):
    """The checks of elmk_set_downscaling_groups: raises ValueError where the device refuses.  Returns (ptr, col, w) as arrays."""
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if ptr.size < 2 or ptr.size - 1 > 2**31 - 1:
        raise ValueError("ngroups outside 1 .. 2^31-1")
    if ptr[0] != 0 or np.any(np.diff(ptr) < 0):
        raise ValueError("ptr must start at 0 and not decrease")
    if ptr[-1] != col.size or col.size != w.size:
        raise ValueError("ptr[-1] must equal len(col) == len(w)")
    if col.size and (col.min() < 0 or col.max() >= ncols):
        raise ValueError("col outside [0, ncols)")
    if np.unique(col).size != col.size:
        raise ValueError("a column in more than one group (or twice in one)")
    if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
        raise ValueError("weights must be finite and >= 0")
    return ptr, col.astype(np.int32), w


def group_norm(lg, lc, ptr, col, w):
    """Per group: norm = (W == 0 || A == 0) ? 1 : (A / W) / (S / W) with W, A, S the aggregates of 1, Lg and Lc (one rounded product
    per term, added in term order).  Returns float64 [ngroups]."""
    ptr, col, w = check_groups(ptr, col, w, np.asarray(lg).size)
    W = RG.apply_aggregate(ptr, col, w, np.ones(np.asarray(lg).size), 0.0)
    A = RG.apply_aggregate(ptr, col, w, lg, 0.0)
    S = RG.apply_aggregate(ptr, col, w, lc, 0.0)
    with np.errstate(all="ignore"):
        q = (A / W) / (S / W)
    return np.where((W == 0.0) | (A == 0.0), 1.0, q)


def renormalise_longwave(lg, lc, ptr, col, w):
    """Lc after the group renormalisation: Lc * norm of its group for every column of a group, unchanged elsewhere."""
    lc = np.array(lc, dtype=np.float64)
    ptr, col, w = check_groups(ptr, col, w, lc.size)
    norm = group_norm(lg, lc, ptr, col, w)
    lc[col] = lc[col] * np.repeat(norm, np.diff(ptr))
    return lc


def downscale_forcing(off, prec, hc, hf, qsat, lapse=LAPSE, lapse_lw=LAPSE_LW, lw_limit=LW_LIMIT, groups=None):
    """The TOPO step from the OFF step's fields `off` (a dict with forc_tbot, forc_pbot, forc_qbot, forc_lwrad at [ncols]), with the
    longwave renormalised over groups = (ptr, col, w) when given.  Returns the dict of downscale()."""
    out = downscale(off["forc_tbot"], off["forc_pbot"], off["forc_qbot"], off["forc_lwrad"], prec, hc, hf, qsat, lapse, lapse_lw,
                    lw_limit)
    if groups is not None:
        out["forc_lwrad"] = renormalise_longwave(off["forc_lwrad"], out["forc_lwrad"], *groups)
    return out
