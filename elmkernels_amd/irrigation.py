"""Irrigation on the host (include/elmk.h "irrigation"; ELM's demand check of CanopyFluxes and the application of canopy_hydrology's
Irrigation() and ground_flux), in numpy and the host libm only: the restatement of the stage the device performs (k_irrigation.hip),
with the same operation order, and the host-side helpers a driver needs.

    S.irrigation_enable(schedule(irrigated, londeg))
    S.irrigation_init(rate_from_restart, nleft_from_restart)             # or nothing: a cold start is all zeros
    st.timestep7_fused(S, dt); S.irrigation(dt, time_of_day(decday, doy)); kokkos_soil_temperature(S, dt); ...
    S.run(dt, steps, st.RUN_IRRIGATION | ...)                            # the same inside every step of a run
    rate, nleft, qirr = (S.irrigation_read(w) for w in (RATE, NLEFT, QFLX_IRRIG))

    out, rows = step(fields, rows, sched, dt, tod, smpso)

The river supply limit (include/elmk.h "irrigation: river supply limit"; S.irrigation_supply_enable(threshold)) follows the stage:

    rate, (demand, committed, ratio, unmet_sum) = supply_limit(ptr, col, w, area, volr, rows[RATE], rows[NLEFT], dt, thr, unmet_sum,
                                                               qflx_irrig=rows[QFLX_IRRIG])
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


# ---- the river supply limit (include/elmk.h "irrigation: river supply limit"; k_history.hip: k_irrigation_supply) -------------------------------
DEMAND, COMMITTED, RATIO, UNMET_SUM = range(4)  # ELMK_IRRSUP_*
SUPPLY_NROWS = 4


def _canon(v):
    """A NaN is stored into a row as the canonical quiet NaN."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v != v, _NAN, v)


def supply_limit(ptr, col, w, area, volr, rate, nleft, idt, thr, unmet_sum, qflx_irrig=None, dam=None, command=None):
    """S0 - S6 on the host: the launch that follows elmk_irrigation while the limit is on.

    ptr, col, w: the output grid's CSR map (every column in at most one cell); area, volr: the routing's [ncells]; rate, nleft: the
    irrigation's rows after this step's irrigation.step ([ncols]); idt: the step in whole seconds; thr: the threshold; unmet_sum:
    [ncells], the prognostic row; qflx_irrig: the irrigation's QFLX_IRRIG row of this step ([ncols]; None: zeros) - the water applied
    in this step, which the routing has not yet taken out of volr (S2's y).  dam = (tab, res): the reservoirs are on (include/elmk.h
    "reservoirs", D7; tab: routing.reservoir_tables, res: the RES row [ncells]) - a dam cell's storage above SMIN counts as available
    beside the channel's; None: S3 as it is.  command: routing.command_tables' dict, the command areas are on too ("command areas", C6;
    needs dam) - per filled slot in order, the cell's claim times the named dam's storage above SMIN counts as well.  Returns (rate_out, rows): rate_out float64 [ncols], rows float64 [SUPPLY_NROWS, ncells] in the order
    DEMAND, COMMITTED, RATIO, UNMET_SUM.  Nothing is changed in place."""
    from . import regrid

    idt = _whole_dt(idt)
    nspd = (IRRIG_LENGTH + (idt - 1)) // idt
    ptr = np.asarray(ptr, dtype=np.int64).reshape(-1)
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    rate = np.array(rate, dtype=np.float64).reshape(-1)
    nleft = np.asarray(nleft, dtype=np.float64).reshape(-1)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    volr = np.asarray(volr, dtype=np.float64).reshape(-1)
    unmet_sum = np.asarray(unmet_sum, dtype=np.float64).reshape(-1)
    thr = float(thr)
    ncells = ptr.size - 1
    if command is not None and dam is None:
        raise ValueError("supply_limit: command without dam")
    assert area.shape == volr.shape == unmet_sum.shape == (ncells,) and rate.shape == nleft.shape
    with np.errstate(all="ignore"):
        checks = nleft == float(nspd)                                # S0
        x = rate * (float(idt) * nleft)                              # S1
        D = regrid.apply_aggregate(ptr, col, w, np.where(checks, x, 0.0), 0.0)  # S2
        y = (np.zeros_like(rate) if qflx_irrig is None else np.asarray(qflx_irrig, dtype=np.float64).reshape(-1)) * float(idt)
        C = regrid.apply_aggregate(ptr, col, w, np.where(~checks & (nleft > 0.0), x, 0.0) + y, 0.0)
        Vd = (D * 0.001) * area                                      # S3
        Vc = (C * 0.001) * area
        a = volr * (1.0 - thr)
        if dam is not None:  # D7
            r = np.asarray(dam[1], dtype=np.float64).reshape(-1) - dam[0]["SMIN"]
            a = np.where(dam[0]["DAM"], a + np.where(r > 0.0, r, 0.0), a)
            if command is not None:  # C6
                for k in range(command["DAM"].shape[0]):
                    on = command["DAM"][k] >= 0
                    rk = r[np.where(on, command["DAM"][k], 0)]
                    a = np.where(on, a + command["CLAIM"][k] * np.where(rk > 0.0, rk, 0.0), a)
        a = a - Vc
        avail = np.where(a > 0.0, a, 0.0)
        ratio = np.where(Vd > avail, avail / np.where(Vd > avail, Vd, 1.0), 1.0)  # S4 (the division only where it is taken)
        cell_of = np.full(rate.size, -1, np.int64)                   # S5: a column in no cell is not limited
        cell_of[col] = np.repeat(np.arange(ncells), np.diff(ptr))
        r = np.where(cell_of >= 0, ratio[np.maximum(cell_of, 0)], 1.0)
        scale = checks & (r != 1.0)
        rate_out = np.where(scale, _canon(rate * r), rate)
        rows = np.stack([_canon(Vd), _canon(Vc), _canon(ratio), _canon(unmet_sum + (Vd - Vd * ratio))])  # S6
    return rate_out, rows
