"""The generated tier of the irrigation tests, host and device: columns that take every branch of the stage over fifty chained steps,
the chain's times of day, and the plant types' smpso; the check's formula in plain floats; and the edge tier: columns that hold one
edge value each beside ordinary ones, the seeds and the times of day of its short chain, and the census that shows what a chain held."""
import math
import os

import numpy as np

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H

CHAIN_STEPS = 50  # 1800 s steps: a day and two steps
CHAIN_TOD0 = 3 * 3600


def chain_tod(s):
    return (CHAIN_TOD0 + 1800 * s) % 86400


def generated(n, seed):
    """The branch-mix generator's columns (synth.make_state, tier B) arranged so that fifty chained steps of the seven wrappers and the
    stage take every branch of A and B: longitudes every half hour of local time with a few hundred seconds of scatter, so that inside
    one wave some columns check, some apply and some do neither; one column in nine not irrigated; bare and leafless columns; capped
    columns; columns frozen at the top (their window opens at rate +0.0) and below layer 3; saturated columns (unstressed) and columns
    wet on top and dry below (deficit 0 beside deficit > 0); roots in the ten active layers only.  Returns (cols, scal, soil, sched)."""
    cols, scal, soil = synth.make_state(st.field_table() if os.path.exists(L.LIB_PATH) else H.field_table_from_oracle(), n, tier="B", seed=seed)
    c = np.arange(n)
    rng = np.random.default_rng(seed + 5)
    s0 = 5
    dzmm = cols["dz"][:, s0:s0 + 15] * 1.0e3
    watsat = cols["watsat"]
    cols["t_soisno"][:, s0:] = np.maximum(cols["t_soisno"][:, s0:], 276.0)  # thawed, unless set otherwise below
    cols["h2osoi_ice"][:, s0:] = 0.0
    root = rng.uniform(0.02, 1.0, (n, 15))
    root[:, 10:] = 0.0
    root[c % 4 == 1, 1] = 0.0
    cols["rootfr"] = root / root.sum(axis=1, keepdims=True)
    cols["h2osoi_liq"][:, s0:] = rng.uniform(0.15, 0.5, (n, 15)) * watsat * dzmm
    m = c % 7 == 2  # saturated: btran reaches 1
    cols["h2osoi_liq"][m, s0:] = watsat[m] * dzmm[m]
    m = c % 7 == 3  # wet on top, dry below
    cols["h2osoi_liq"][m, s0:s0 + 3] = 0.98 * watsat[m, :3] * dzmm[m, :3]
    cols["t_soisno"][c % 6 == 4, s0] = 272.0  # frozen at the top
    cols["t_soisno"][c % 6 == 5, s0 + 3] = 270.0  # frozen layer 3
    cols["frac_veg_nosno"][:] = np.where(c % 10 == 6, 0, 1)
    cols["frac_veg_nosno_alb"][:] = cols["frac_veg_nosno"]
    cols["elai"][:] = np.where(c % 10 == 8, 0.0, np.maximum(cols["elai"], 0.3))
    cols["esai"][:] = np.maximum(cols["esai"], 0.1)
    cols["do_capsnow"][:] = (c % 5 == 0).astype(np.int32)
    lon = ((c * 7) % 48) * 7.5 - 180.0 + (c % 9) * 0.4  # 0.4 degrees = 96 s
    sched = ir.schedule(c % 9 != 4, lon)
    return cols, scal, soil, sched


def smpso_of(vtype):
    pft, _ = synth.load_params()
    return np.asarray(pft["smpso"], dtype=np.float64).reshape(-1)[np.asarray(vtype)]


def rate_by_hand(f, c, nlayers, dt, smpso=-66000.0):
    """The check's formula written out in plain floats, over soil layers 0 .. nlayers - 1 of column c that have roots (well-formed
    columns only: Python's own pow, / and max)."""
    nspd = (14400 + (int(dt) - 1)) // int(dt)
    rate = 0.0
    for j in range(nlayers):
        if not f["rootfr"][c, j] > 0.0:
            continue
        ep, dz = float(f["eff_porosity"][c, j]), float(f["dz"][c, 5 + j])
        vol_liq_so = ep * math.pow(-smpso / float(f["sucsat"][c, j]), -1.0 / float(f["bsw"][c, j]))
        liq_so = vol_liq_so * 1000.0 * dz
        liq_sat = ep * 1000.0 * dz
        deficit = max((liq_so + 0.7 * (liq_sat - liq_so)) - float(f["h2osoi_liq"][c, 5 + j]), 0.0)
        rate = rate + deficit / (dt * nspd)
    return rate


# ---- the edge tier ------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
DTS = (1, 1800, 3600, 7000, 14400, 14401, 86400)  # nspd 14400, 8, 4, 3 (no divisor of the window), 1, 1 (longer than the window), 1
EDGE_VALUES = (0.0, -0.0, -3.5, 5e-324, 1e300, NAN, INF, -INF)  # E
# (field, level): soil layer j is level 5 + j of t_soisno, dz and h2osoi_liq and level j of the others
EDGE_SLOTS = (("t_soisno", 5 + 0), ("t_soisno", 5 + 7), ("rootfr", 2), ("eff_porosity", 2), ("sucsat", 2), ("bsw", 2), ("dz", 5 + 2),
              ("h2osoi_liq", 5 + 2), ("btran", None), ("elai", None))
CLOCK_SCHED = (0, 1, 21600, 64800, 86399)
APPLY_CAPSNOW = (0, 1, -1, 2)
APPLY_TARGET = (-0.0, 1e300, INF, -INF, NAN)
APPLY_RATE = (5e-324, 1e300, 2.5e-4)
N_APPLY = 20  # k % 3 and k // 3 % 3 take the nine (NLEFT, RATE) pairs in k = 0 .. 8, k % 4 and k % 5 the twenty (do_capsnow, target) pairs
ORDINARY_RATE = 1.5e-4


def edge_classes():
    """The edge columns in the order they are laid out: [(name, field, level, value)].  Class k sits in column 2 k.  An applying
    class has field "apply" and value k: its do_capsnow, target field and target value follow from k (APPLY_*), its rows from edge_seed.
    The plant types' table has one type whose smpso is 0 (type 0, bare ground), so the smpso class is in."""
    out = [(f"{f}[{lev}]={v!r}", f, lev, v) for f, lev in EDGE_SLOTS for v in EDGE_VALUES]
    out += [("t_soisno[8]=TFRZ", "t_soisno", 5 + 3, ir.TFRZ), ("t_soisno[8]=TFRZ+", "t_soisno", 5 + 3, float(np.nextafter(ir.TFRZ, INF))),
            ("btran=thresh", "btran", None, ir.IRRIG_BTRAN_THRESH), ("btran=thresh-", "btran", None, float(np.nextafter(ir.IRRIG_BTRAN_THRESH, 0.0))),
            ("elai=5e-324", "elai", None, 5e-324), ("frac_veg_nosno=-1", "frac_veg_nosno", None, -1), ("frac_veg_nosno=2", "frac_veg_nosno", None, 2)]
    out += [(f"apply{k}", "apply", None, k) for k in range(N_APPLY)]
    pft, _ = synth.load_params()
    zero = np.nonzero(np.asarray(pft["smpso"], dtype=np.float64).reshape(-1) == 0.0)[0]
    if zero.size:
        out.append(("smpso=0", "vtype", None, int(zero[0])))
    return out


def edge_index(name, n):
    """The column of the edge class `name` (None where n columns do not reach it)."""
    k = [c[0] for c in edge_classes()].index(name)
    return 2 * k if 2 * k < n else None


def edge_tier(n, seed):
    """The generated tier's columns with the edge tier written over them.  Returns (cols, scal, soil, sched).

    Even columns 0, 2, .. are the edge columns, class k in column 2 k as far as n allows (257 columns hold every class): irrigated,
    vegetated, leafy, stressed (btran 0.3), thawed, rooted in layers 0 .. 9, sched 0 - on the clock at tod 21600 - and one input
    replaced by the class's value.  The columns between them and after them are ordinary ones: every branch of A and B on well-formed
    values (bare, leafless, unstressed, not irrigated, frozen, rootless, saturated, capped), their sched dealt from CLOCK_SCHED, so
    that a 64-column wave holds edge columns and ordinary ones, columns that check, that apply and that do neither.  No wrapper may
    run between the upload and elmk_irrigation: the seven wrappers overwrite btran and the two precipitation terms."""
    cols, scal, soil, _ = generated(n, seed)
    c = np.arange(n)
    k = c // 2
    sched = np.asarray(CLOCK_SCHED, np.int32)[k % 5].copy()
    sched[k % 18 == 17] = -1
    # what the wrappers would have left: btran, and the two precipitation terms
    cols["btran"] = np.where(k % 7 == 2, 1.0, 0.3 + 0.001 * (c % 50))
    cols["frac_veg_nosno"][:] = np.where(k % 10 == 6, 0, 1)
    cols["frac_veg_nosno_alb"][:] = cols["frac_veg_nosno"]
    cols["elai"][:] = np.where(k % 10 == 8, 0.0, np.maximum(cols["elai"], 0.3))
    cols["do_capsnow"][:] = (k % 5 == 0).astype(np.int32)
    cols["rootfr"][k % 4 == 1, 1] = 0.0
    cols["t_soisno"][k % 6 == 4, 5] = 272.0
    cols["t_soisno"][k % 6 == 5, 5 + 3] = 270.0
    cols["qflx_rain_grnd"] = 1.0e-5 * (1 + c % 7).astype(np.float64)
    cols["qflx_snwcp_liq"] = 1.0e-6 * (c % 3).astype(np.float64)
    for kk, (name, field, lev, v) in enumerate(edge_classes()):
        i = 2 * kk
        if i >= n:
            break
        sched[i] = 0
        cols["frac_veg_nosno"][i] = cols["frac_veg_nosno_alb"][i] = 1
        cols["elai"][i], cols["btran"][i], cols["do_capsnow"][i] = 2.0, 0.3, 0
        cols["t_soisno"][i, 5:] = np.maximum(cols["t_soisno"][i, 5:], 276.0)
        cols["rootfr"][i, :10] = np.maximum(cols["rootfr"][i, :10], 0.01)
        if field == "apply":
            cap = APPLY_CAPSNOW[v % 4]
            cols["do_capsnow"][i] = cap
            cols["qflx_snwcp_liq" if cap != 0 else "qflx_rain_grnd"][i] = APPLY_TARGET[v % 5]
        elif lev is None:
            cols[field][i] = v
        else:
            cols[field][i, lev] = v
    return cols, scal, soil, sched


def edge_seed(n, dt):
    """RATE and NLEFT for elmk_irrigation_init (which accepts them: finite, non-negative rates, whole NLEFT): the applying classes'
    NLEFT in {1, 2, nspd} and RATE in APPLY_RATE, and an open window on one ordinary column in four."""
    nspd = ir.steps_per_day(dt)
    c = np.arange(n)
    rate = np.where((c % 2 == 1) & (c // 2 % 4 == 1), 1.0e-4 + 1.0e-6 * (c % 97), 0.0)
    nleft = np.where(rate > 0.0, 3.0, 0.0)
    for k in range(N_APPLY):
        i = edge_index(f"apply{k}", n)
        if i is not None:
            nleft[i] = (1.0, 2.0, float(nspd))[k % 3]
            rate[i] = APPLY_RATE[k // 3 % 3]
    return rate, nleft


def clock_tods(idt):
    """The times of day of a short chain.  For a sched 0 column: since = 0, idt - 1 and (idt < 86400) idt; then tod = 21599 (since
    86399), 86399 and 0; then 43200 and 21601, at which the sched 64800 and sched 86399 columns check with tod + sched >= 86400."""
    tods = [ir.IRRIG_START, (ir.IRRIG_START + idt - 1) % ir.DAY]
    if idt < ir.DAY:
        tods.append((ir.IRRIG_START + idt) % ir.DAY)
    return tods + [21599, 86399, 0, 43200, 21601]


EDGE_CENSUS = ir.BRANCHES + ("rate_nan", "rate_inf", "rate_huge", "rate_subnormal", "apply_nan", "apply_inf", "target_nonfinite", "break_at_tfrz",
                             "btran_at_threshold", "since_zero", "since_last_in", "since_first_out", "local_wrapped", "recheck_in_open_window",
                             "window_ran_out")


def _as_stored(v, stored):
    """The value a context holds after v was uploaded: v itself, or v rounded to the fp32 state's type."""
    return v if stored is None else float(stored(v))


def edge_step(seen, fields, rows, sched, dt, tod, smpso, stored=None):
    """irrigation.step on what a context holds, and the census of the call added to `seen` (name -> count over EDGE_CENSUS), from the
    inputs and the restatement's outputs alone.  Returns irrigation.step's (out, rows_out).

    rate_*: values of the RATE row before or after the call (huge: finite and >= 1e290).  apply_nan: NLEFT > 0 and RATE NaN -
    QFLX_IRRIG is the canonical NaN and neither state field moves (counted only where both hold); apply_inf: the same with +inf;
    target_nonfinite: water is added to a field that holds a NaN or an infinity.  break_at_tfrz: a checking column leaves the loop at
    a layer that holds tfrz as the context stores it (273.15, or its fp32 neighbour below); btran_at_threshold: an otherwise eligible
    column holds 0.999999 as stored (not stressed in the fp64 build; its fp32 neighbour lies below and is stressed).  since_*: an eligible column with since = 0, idt - 1 (both check) or idt (does not); local_wrapped: a checking
    column with tod + sched >= 86400.  recheck_in_open_window: NLEFT > 0 before and the column checks; window_ran_out: A brings
    NLEFT to 0."""
    idt = int(dt)
    nspd = ir.steps_per_day(dt)
    out, rows_out = ir.step(fields, rows, sched, dt, tod, smpso, stored=stored, hit=seen)
    f = {k: np.asarray(fields[k]) for k in ir.READS}
    rows = np.asarray(rows, dtype=np.float64)
    sched = np.asarray(sched, dtype=np.int64)
    on = rows[ir.NLEFT] > 0.0
    rate0 = rows[ir.RATE]
    add = lambda name, m: seen.__setitem__(name, seen.get(name, 0) + int(np.sum(m)))  # noqa: E731
    with np.errstate(all="ignore"):
        both = np.concatenate([rate0, rows_out[ir.RATE]])
        add("rate_nan", np.isnan(both))
        add("rate_inf", np.isinf(both))
        add("rate_huge", np.isfinite(both) & (np.abs(both) >= 1.0e290))
        add("rate_subnormal", (both != 0.0) & (np.abs(both) < 2.2250738585072014e-308))
        untouched = np.ones(rate0.size, bool)
        for k in ir.WRITES:
            untouched &= _rows_equal(out[k], f[k])
        add("apply_nan", on & np.isnan(rate0) & untouched & (rows_out[ir.QFLX_IRRIG].view(np.uint64) == np.uint64(0x7FF8000000000000)))
        add("apply_inf", on & (rate0 == INF))
        cap = f["do_capsnow"].reshape(-1) != 0
        target = np.where(cap, f["qflx_snwcp_liq"].astype(np.float64).reshape(-1), f["qflx_rain_grnd"].astype(np.float64).reshape(-1))
        add("target_nonfinite", on & (rate0 > 0.0) & ~np.isfinite(target))
        add("window_ran_out", on & (rows[ir.NLEFT] - 1.0 == 0.0))
        # the seeds never exceed nspd and A counts down first, so after the call NLEFT == nspd exactly where B ran (S0's marker)
        checks = rows_out[ir.NLEFT] == float(nspd)
        btran = f["btran"].astype(np.float64).reshape(-1)
        rest = (sched >= 0) & (f["frac_veg_nosno"].reshape(-1) != 0) & (f["elai"].astype(np.float64).reshape(-1) > 0.0)
        eligible = rest & (btran < ir.IRRIG_BTRAN_THRESH)
        since = ir.seconds_since_start(np.maximum(sched, 0), tod)
        add("btran_at_threshold", rest & (btran == _as_stored(ir.IRRIG_BTRAN_THRESH, stored)))
        add("since_zero", checks & (since == 0))
        add("since_last_in", checks & (since == idt - 1))
        add("since_first_out", eligible & ~checks & (since == idt))
        add("local_wrapped", checks & (int(tod) + sched >= ir.DAY))
        add("recheck_in_open_window", on & checks)
        t = f["t_soisno"].astype(np.float64)[:, ir.NLEVSNO:ir.NLEVSNO + ir.NLEVGRND]
        frozen = t <= ir.TFRZ
        first = np.argmax(frozen, axis=1)
        at = t[np.arange(rate0.size), first] == _as_stored(ir.TFRZ, stored)
        add("break_at_tfrz", checks & frozen.any(axis=1) & at)
    return out, rows_out


def _rows_equal(a, b):
    """Per column: the same bytes."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.dtype == b.dtype
    w = a.itemsize
    return (a.view(np.uint8).reshape(-1, w) == b.view(np.uint8).reshape(-1, w)).all(axis=1)


def census_missing(seen, dt):
    """The names of EDGE_CENSUS a chain left empty, after the one exemption.  (The fp32-state build stores 1e300 as inf and 5e-324 as
    0, so no check there produces a huge or a subnormal rate from such a field; the seeded rows are fp64 in both builds and keep
    rate_huge and rate_subnormal filled, so they are not exempt.)"""
    missing = {k for k in EDGE_CENSUS if not seen.get(k)}
    if int(dt) == ir.DAY:
        # a step of a whole day holds every local 06:00: since < 86400 always, no clock is out
        missing -= {"off_clock", "since_first_out"}
    return missing
