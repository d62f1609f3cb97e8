"""Active layer thickness on the host (include/elmk.h "active layer thickness"; ELM's ActiveLayerMod::alt_calc), in numpy only: the
restatement of the update the device performs (k_active_layer.hip), with the same operation order, and the run's rollover rule.

    S.active_layer_enable()
    S.active_layer_init(altmax_from_restart, altmax_lastyear_from_restart)   # the indices come in through S["altmax_indx"] = ...
    S.run(dt, steps, st.RUN_ALT)                                             # every step: physics, then the update
    alt, altmax, altmax_lastyear = (S.active_layer_read(w) for w in (ALT, ALTMAX, ALTMAX_LASTYEAR))

    update(t_soisno, zsoi, alt, altmax, altmax_lastyear, altmax_indx, altmax_lastyear_indx, north, rollover(doy, decday))

The indices are 0-based soil-layer numbers with -1 for "no thawed layer" (ELM's index minus one), which is how
normalize_unfrozen_rootfr reads them.
"""
import numpy as np

ALT, ALTMAX, ALTMAX_LASTYEAR = range(3)  # ELMK_ALT_*
ROLL_NORTH, ROLL_SOUTH = 1, 2  # ELMK_ALT_ROLL_*
TFRZ = 273.15
NLEVSNO, NLEVGRND = 5, 15  # level NLEVSNO + j of t_soisno / zsoi is soil layer j


def rollover(doy, decday):
    """The rollover bits of the elmk_run step that starts at (doy, decday) - elmk_run_step's fields, decday = decimal day of year + 1:
    NORTH for the step that starts at 00:00 of 1 January, SOUTH for the one that starts at 00:00 of 1 July of the no-leap calendar
    (the steps whose end-of-step date satisfies ELM's mon, day == 1 and sec / dtime == 1)."""
    return (ROLL_NORTH if int(doy) == 0 and float(decday) == 1.0 else 0) | (ROLL_SOUTH if int(doy) == 181 and float(decday) == 182.0 else 0)


def north(lat_r):
    """Which columns count as northern: sin(lat) > 0.0, as the device reads it from the column geography (lat == 0 goes south)."""
    return np.sin(np.asarray(lat_r, dtype=np.float64)) > 0.0


def update(t_soisno, zsoi, alt, altmax, altmax_lastyear, altmax_indx, altmax_lastyear_indx, north, rollover=0, inplace=False):  # noqa: A002
    """One elmk_active_layer_update.  t_soisno, zsoi: [20, n] (any float dtype, widened to fp64); alt, altmax, altmax_lastyear: [n]
    fp64; altmax_indx, altmax_lastyear_indx: [n] int32; north: [n] bool; rollover: ROLL_* bits.  Returns the five arrays (alt, altmax,
    altmax_lastyear, altmax_indx, altmax_lastyear_indx) after the update; with inplace they are the arguments, written in place.
    Every operation is one IEEE fp64 operation, in the order of include/elmk.h; numpy fuses nothing."""
    rollover = int(rollover)
    if rollover & ~(ROLL_NORTH | ROLL_SOUTH):
        raise ValueError("active_layer.update: unknown rollover bits")
    t = np.asarray(t_soisno).astype(np.float64)[NLEVSNO:NLEVSNO + NLEVGRND]
    z = np.asarray(zsoi).astype(np.float64)[NLEVSNO:NLEVSNO + NLEVGRND]
    n = t.shape[1]
    north = np.asarray(north, dtype=bool)
    if not inplace:
        alt, altmax, altmax_lastyear = (np.array(a, dtype=np.float64) for a in (alt, altmax, altmax_lastyear))
        altmax_indx, altmax_lastyear_indx = (np.array(a, dtype=np.int32) for a in (altmax_indx, altmax_lastyear_indx))
    roll = ((rollover & ROLL_NORTH) != 0) & north | ((rollover & ROLL_SOUTH) != 0) & ~north
    altmax_lastyear[roll] = altmax[roll]
    altmax_lastyear_indx[roll] = altmax_indx[roll]
    altmax[roll] = 0.0
    altmax_indx[roll] = -1
    with np.errstate(all="ignore"):
        thawed = t > TFRZ  # a NaN is not thawed
        bottom = thawed[NLEVGRND - 1]
        # the largest j in 0 .. 13 that is thawed, or -1
        j = np.arange(NLEVGRND - 1)[:, None]
        k = np.where(thawed[:NLEVGRND - 1], j, -1).max(axis=0)
        kk = np.maximum(k, 0)
        cols = np.arange(n)
        z1, z2, t1, t2 = z[kk, cols], z[kk + 1, cols], t[kk, cols], t[kk + 1, cols]
        a = z1 + ((t1 - TFRZ) * (z2 - z1)) / (t1 - t2)
        a = np.where(k >= 0, a, 0.0)
        a = np.where(bottom, z[NLEVGRND - 1], a)
        a = np.where(np.isnan(a), np.float64(np.nan), a)  # one NaN (0x7FF8000000000000), whatever sign and payload the operations gave
        k = np.where(bottom, NLEVGRND - 1, k).astype(np.int32)
        alt[...] = a
        grow = a > altmax
    altmax[grow] = a[grow]
    altmax_indx[grow] = k[grow]
    return alt, altmax, altmax_lastyear, altmax_indx, altmax_lastyear_indx


def cold_start(S):
    """A cold start on an ELMState with the feature enabled: the three rows zero, both index fields -1."""
    S.active_layer_init(None, None)
    S["altmax_indx"] = np.full(S.ncols, -1, np.int32)
    S["altmax_lastyear_indx"] = np.full(S.ncols, -1, np.int32)
