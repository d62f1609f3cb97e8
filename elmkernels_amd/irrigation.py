"""Irrigation on the host (include/elmk.h "irrigation"; ELM's demand check of CanopyFluxes and the application of canopy_hydrology's
Irrigation() and ground_flux), in numpy and the host libm only: the restatement of the stage the device performs (k_irrigation.hip),
with the same operation order, and the host-side helpers a driver needs.

    S.irrigation_enable(schedule(irrigated, londeg))
    S.irrigation_init(rate_from_restart, nleft_from_restart)             # or nothing: a cold start is all zeros
    st.timestep7_fused(S, dt); S.irrigation(dt, time_of_day(decday, doy)); kokkos_soil_temperature(S, dt); ...
    S.run(dt, steps, st.RUN_IRRIGATION | ...)                            # the same inside every step of a run
    rate, nleft, qirr = (S.irrigation_read(w) for w in (RATE, NLEFT, QFLX_IRRIG))

    out, rows = step(fields, rows, sched, dt, tod, smpso)
"""
import math

import numpy as np

from .hydrology import _div, _max, _pow

RATE, NLEFT, QFLX_IRRIG = range(3)  # ELMK_IRR_*
NROWS = 3
NOT_IRRIGATED = -1  # sched
IRRIG_FACTOR, IRRIG_MIN_LAI, IRRIG_BTRAN_THRESH = 0.7, 0.0, 0.999999
IRRIG_START, IRRIG_LENGTH, DAY = 21600, 14400, 86400  # 06:00 local time, four hours
DEGPSEC = 15.0 / 3600.0  # degrees of longitude per second of local time
TFRZ, DENH2O = 273.15, 1000.0
NLEVSNO, NLEVGRND = 5, 15  # level NLEVSNO + j of t_soisno / h2osoi_liq / dz is soil layer j
# the state fields the stage reads, and the two it changes
READS = ("do_capsnow", "qflx_rain_grnd", "qflx_snwcp_liq", "frac_veg_nosno", "elai", "btran", "t_soisno", "rootfr", "eff_porosity",
         "sucsat", "bsw", "dz", "h2osoi_liq")
WRITES = ("qflx_rain_grnd", "qflx_snwcp_liq")
# the branches of A and B a column can take (step's census)
BRANCHES = ("apply_capped", "apply_uncapped", "apply_zero", "idle", "not_irrigated", "no_veg", "no_lai", "unstressed", "off_clock", "check",
            "frozen_break", "rootless_layer", "deficit_positive", "deficit_zero")
_NAN = float(np.float64(np.nan))


def _round_half_away(x):
    """C's round(): to the nearest whole number, halves away from zero."""
    x = float(x)
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 2.0 ** 52 else x


def schedule(irrigated, londeg):
    """The int32 parameter row of elmk_irrigation_enable: -1 where the column is not irrigated, else its longitude offset in seconds
    normalised to 0 .. 86399 - ELM's round(londeg / degpsec), degpsec = 15 / 3600, halves away from zero, reduced mod 86400."""
    irrigated = np.asarray(irrigated, dtype=bool).reshape(-1)
    lon = np.broadcast_to(np.asarray(londeg, dtype=np.float64).reshape(-1), irrigated.shape)
    out = np.full(irrigated.size, NOT_IRRIGATED, np.int32)
    for i in np.nonzero(irrigated)[0]:
        out[i] = int(_round_half_away(float(lon[i]) / DEGPSEC)) % DAY
    return out


def time_of_day(decday, doy):
    """Seconds after midnight UTC at the start of the step that starts at (doy, decday) - elmk_run_step's fields, decday = decimal day
    of year + 1: llround((decday - 1.0 - doy) * 86400.0) reduced to 0 .. 86399, as elmk_run derives it."""
    return int(_round_half_away((float(decday) - 1.0 - float(int(doy))) * 86400.0)) % DAY


def steps_per_day(dt):
    """The steps of the four-hour window: (14400 + (idt - 1)) / idt in integer division."""
    idt = _whole_dt(dt)
    return (IRRIG_LENGTH + (idt - 1)) // idt


def _whole_dt(dt):
    idt = int(dt)
    if float(dt) != float(idt) or not 1 <= idt <= DAY:
        raise ValueError("irrigation: dt must be a whole number of seconds in 1 .. 86400")
    return idt


def seconds_since_start(sched, tod):
    """since of B: the seconds the column's local clock is past 06:00 at the step's start; the column checks in the step with since < idt."""
    local = (int(tod) + np.asarray(sched, dtype=np.int64)) % DAY
    return (local - IRRIG_START + DAY) % DAY


def check_rate(t, rootfr, effpor, sucsat, bsw, dz, liq, smpso, dtn, hit=None):
    """B's loop for one column, from fifteen-element lists of fp64 values (soil layers 0 .. 14): the new RATE.  dtn = dt * nspd."""
    rate = 0.0
    for j in range(NLEVGRND):
        if t[j] <= TFRZ:
            _hit(hit, "frozen_break")
            break
        if rootfr[j] > 0.0:
            vol_liq_so = effpor[j] * _pow(_div(-smpso, sucsat[j]), _div(-1.0, bsw[j]))
            liq_so = vol_liq_so * DENH2O * dz[j]
            liq_sat = effpor[j] * DENH2O * dz[j]
            deficit = _max((liq_so + IRRIG_FACTOR * (liq_sat - liq_so)) - liq[j], 0.0)
            _hit(hit, "deficit_positive" if deficit > 0.0 else "deficit_zero")
            rate = rate + _div(deficit, dtn)
        else:
            _hit(hit, "rootless_layer")
    return _NAN if rate != rate else rate


def _hit(hit, name):
    if hit is not None:
        hit[name] = hit.get(name, 0) + 1


def step(fields, rows, sched, dt, tod, smpso, stored=None, hit=None):
    """One elmk_irrigation on the host.

    fields: a dict of the state fields READS as S[name] downloads them ([n] or [n, nlev]; float fields of any float dtype, widened to
    fp64 as stored); rows: float64 [NROWS, n], the rows of the feature; sched: int32 [n]; dt: the step, a whole number of seconds; tod:
    seconds after midnight UTC at the step's start; smpso: the PFT parameter, a scalar or [n] (the value of each column's vtype).
    Returns (out, rows_out): out holds the fields WRITES in the dtype of the inputs (the sum rounded once to the stored type), rows_out
    the rows after the step.  Nothing is changed in place.  stored: the element type the state is stored in where the inputs do not
    show it - np.float32 for downloads of the fp32-state build.  hit: a dict that counts the BRANCHES the columns take."""
    idt = _whole_dt(dt)
    tod = int(tod)
    if not 0 <= tod < DAY:
        raise ValueError("irrigation.step: tod outside 0 .. 86399")
    nspd = (IRRIG_LENGTH + (idt - 1)) // idt
    f = {k: np.asarray(fields[k]) for k in READS}
    rows_out = np.array(rows, dtype=np.float64)
    n = rows_out.shape[1]
    assert rows_out.shape == (NROWS, n)
    sched = np.asarray(sched, dtype=np.int32).reshape(-1)
    assert sched.shape == (n,)
    smpso = np.broadcast_to(np.asarray(smpso, dtype=np.float64), (n,))
    out = {k: np.array(f[k]) for k in WRITES}

    with np.errstate(all="ignore"):
        # A: apply
        nleft, rate = rows_out[NLEFT].copy(), rows_out[RATE].copy()
        on = nleft > 0.0
        q = np.where(on, rate, 0.0)
        rows_out[NLEFT] = np.where(on, nleft - 1.0, nleft)
        rows_out[QFLX_IRRIG] = np.where(q != q, _NAN, q)
        pos = q > 0.0
        cap = np.asarray(f["do_capsnow"]).reshape(-1) != 0
        for name, mask in (("qflx_snwcp_liq", pos & cap), ("qflx_rain_grnd", pos & ~cap)):
            total = f[name].astype(np.float64).reshape(-1) + q
            total = (total if stored is None else total.astype(stored)).astype(out[name].dtype)
            out[name] = np.where(mask.reshape(out[name].shape), total.reshape(out[name].shape), out[name])
        if hit is not None:
            for name, m in (("apply_capped", pos & cap), ("apply_uncapped", pos & ~cap), ("apply_zero", on & ~pos), ("idle", ~on)):
                hit[name] = hit.get(name, 0) + int(m.sum())

        # B: check
        fvn = np.asarray(f["frac_veg_nosno"]).reshape(-1) != 0
        elai = f["elai"].astype(np.float64).reshape(-1) > IRRIG_MIN_LAI
        stressed = f["btran"].astype(np.float64).reshape(-1) < IRRIG_BTRAN_THRESH
        irrigated = sched >= 0
        clock = seconds_since_start(np.maximum(sched, 0), tod) < idt
        if hit is not None:
            for name, m in (("not_irrigated", ~irrigated), ("no_veg", irrigated & ~fvn), ("no_lai", irrigated & fvn & ~elai),
                            ("unstressed", irrigated & fvn & elai & ~stressed), ("off_clock", irrigated & fvn & elai & stressed & ~clock)):
                hit[name] = hit.get(name, 0) + int(m.sum())
        checks = np.nonzero(irrigated & fvn & elai & stressed & clock)[0]
    if checks.size:
        s0, s1 = NLEVSNO, NLEVSNO + NLEVGRND
        w = {k: f[k][checks].astype(np.float64) for k in ("t_soisno", "rootfr", "eff_porosity", "sucsat", "bsw", "dz", "h2osoi_liq")}
        dtn = float(idt) * float(nspd)
        for i, c in enumerate(checks):
            _hit(hit, "check")
            rows_out[NLEFT, c] = float(nspd)
            rows_out[RATE, c] = check_rate(w["t_soisno"][i, s0:s1].tolist(), w["rootfr"][i, :NLEVGRND].tolist(),
                                           w["eff_porosity"][i, :NLEVGRND].tolist(), w["sucsat"][i, :NLEVGRND].tolist(),
                                           w["bsw"][i, :NLEVGRND].tolist(), w["dz"][i, s0:s1].tolist(), w["h2osoi_liq"][i, s0:s1].tolist(),
                                           float(smpso[c]), dtn, hit)
    return out, rows_out
