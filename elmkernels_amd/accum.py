"""Accumulated fields on the host (include/elmk.h "accumulated fields"; ELM's accumulMod), in numpy only: the restatement of the
update the device performs (k_accum.hip), with the same operation order, and the helpers a driver needs to register ELM's fields.

    e = accum.add_t10(S, dt)                 # T10: running mean of t_ref2m over 10 days, written to t10
    S.accum_init(e, t10_from_restart, nstep) # or S.accum_init(e): seeded from the t10 that was uploaded
    S.run(dt, steps, st.RUN_ACCUM)           # every step: physics, then the update, then the history

    val = accum.update(val, v, kind, period, nstep)    # what one elmk_accum_update does to an entry, bit for bit
"""
import numpy as np

RUNMEAN, TIMEAVG, RUNACCUM = range(3)  # ELMK_ACCUM_*
KINDS = {"runmean": RUNMEAN, "timeavg": TIMEAVG, "runaccum": RUNACCUM}
MAX_ENTRIES = 16
SPVAL_RESET = -99999.0  # RUNACCUM: a sample that rounds to it resets the accumulation (accumulMod's accumresetval)
RUNACCUM_MAX = 99999.0
T10_DAYS = 10


def update(val, v, kind, period, nstep):
    """One update of an entry: val the fp64 value before it, v the samples (any dtype, widened to fp64), nstep = n + 1 with n the
    updates folded in so far.  Returns the new value (val is not modified).  Every operation is one IEEE fp64 operation, in the
    order of include/elmk.h; numpy fuses nothing."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    period, nstep = int(period), int(nstep)
    if period < 1 or nstep < 1:
        raise ValueError("accum.update: period and nstep start at 1")
    val = np.asarray(val, dtype=np.float64)
    v = np.asarray(v).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == RUNMEAN:
            a = min(nstep, period)
            return (np.float64(a - 1) * val + v) / np.float64(a)
        if kind == TIMEAVG:
            if nstep % period == 1 or period == 1:
                val = np.zeros_like(val)
            val = val + v
            if nstep % period == 0:
                val = val / np.float64(period)
            return val
        if kind == RUNACCUM:
            t = val + v
            t = np.where(t > 0.0, t, 0.0)
            t = np.where(t < RUNACCUM_MAX, t, RUNACCUM_MAX)
            return np.where(np.rint(v) == SPVAL_RESET, 0.0, t)
    raise ValueError(f"accum.update: unknown kind {kind}")


def writes_destination(kind, period, nstep):
    """Whether the update with this nstep writes the destination field: always, except TIMEAVG inside a period."""
    kind = KINDS[kind] if isinstance(kind, str) else int(kind)
    return kind != TIMEAVG or int(nstep) % int(period) == 0


def period_steps(period, dt):
    """ELM's accumulation period in steps: a positive period is a number of steps, a negative one a number of days (accumulMod's
    init_accum_field).  A period of days must be a whole number of steps of dt seconds."""
    dt = float(dt)
    if not (dt > 0.0 and np.isfinite(dt)):
        raise ValueError("accum.period_steps: dt must be finite and positive")
    if period != int(period) or int(period) == 0:
        raise ValueError("accum.period_steps: the period is a non-zero whole number (steps, or days if negative)")
    period = int(period)
    if period > 0:
        return period
    steps = -period * 86400.0 / dt
    if steps != np.floor(steps) or steps < 1:
        raise ValueError(f"accum.period_steps: {-period} days are not a whole number of steps of {dt} s")
    return int(steps)


def add_t10(S, dt, period=-T10_DAYS):
    """Register ELM's T10 on an ELMState: the running mean of t_ref2m over `period` (as period_steps reads it: -10 is ten days of
    steps of dt seconds), written to t10, which canopy_fluxes reads for the acclimation of photosynthesis.  Returns the entry id."""
    return S.accum_add("t_ref2m", RUNMEAN, period_steps(period, dt), "t10")
