"""The "full step" case that the host and device tests of the whole run step share: one small context with every optional part of
elmk_run's step switched on at once - all nine run flags, the frost table, the irrigation with its river supply limit, the routing with
the withdrawal, the kinematic-wave scheme and its floodplain inundation, COSZEN shortwave, TOPO downscaling with longwave groups, an
aerosol series, the active layer, history entries with every op on two tapes and over a row of every feature family per column and
gridded, two accumulator entries - the same steps through the stand-alone calls in RUN_STEP's order (api_run.cpp), and a snapshot of
everything the device holds that a step can change.

The sizes are the smallest that still reach every path: 193 columns (no multiple of 64, under one workgroup of most kernels plus a
ragged tail) of the irrigation's generated tier on the soil land unit with the hydrology's prepared rows and the permafrost tier on
top; 70 cells (cld 128: a second 64-block that holds six cells) with empty cells, a single-column cell and free columns; network A with
in-degree 8 and upstream cells on both sides of the hub (npad 8), network B a chain (npad 1); nsub 3 (odd: the linear scheme starts in
its second buffer) and 2.

The forcing grid stays out of this case: it changes the layout of the uploaded series, and test_gpu_forcing_grid.py owns the
equivalence of gridded and per-column series.

`geometry()` is numpy alone (the host test reads nothing else); `case()` adds the state and needs the library's field table."""
import functools

import numpy as np

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import regrid as RG
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc
from tests.support import same

NCOL, NCELL = 193, 70
NSTEPS, HALF = 12, 6
NREC = 10
DT = 1800.0
SEED = 900
TOL, THR = 1.0e-9, 0.1
NSUB_A, NSUB_B = 3, 2
NAN = float("nan")
FORC_DT = 3600.0
REC_TIMES = 14.875 + np.arange(NREC) / 24.0  # the hourly records of run_cases.schedule(), which starts at 21:00 of day 13
ALL_FLAGS = (st.RUN_QBOT_IS_RH | st.RUN_HISTORY | st.RUN_ACCUM | st.RUN_AEROSOL | st.RUN_ALT | st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE |
             st.RUN_IRRIGATION | st.RUN_ROUTING)
ROUTE_ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR, rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC)
SUP_ROWS = (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)
FIELD_ENTRIES = ((0, "t_grnd", "avg"), (0, "eflx_sh_tot", "sum"), (0, "t_soisno", "max"), (1, "h2osoi_liq", "min"), (1, "snl", "inst"))
# one row of each family: per column on one tape, gridded on the other
ROW_ENTRIES = (("alt", st.ALT_ALT), ("hydrology", hy.ZWT), ("frost", hy.QFLX_DRAIN_PERCHED), ("water_balance", hy.WB_QRUNOFF),
               ("irrigation", ir.QFLX_IRRIG))
ROW_FAMILIES = tuple(f for f, _ in ROW_ENTRIES)
ACCUM_ENTRIES = (("t_grnd", "runmean", 3), ("h2osoi_liq", "timeavg", 2))
AEROSOL_STREAMS = ("bcphi", "dst4_2")
# the columns never irrigated, and the irrigated ones whose local 06:00 lies outside the twelve steps
LATE = 16


# ---- numpy alone: the cells, the networks, the schedules ---------------------------------------------------------------------------
def irrigation_sched():
    """Column c passes 06:00 local time in step c % 16 of run_cases.schedule() (so one column in four never does in twelve steps), with
    up to 400 s of scatter inside the step; one column in seven is not irrigated."""
    c = np.arange(NCOL)
    sched = ((32400 - 1800 * (c % LATE) + 100 * (c % 5)) % 86400).astype(np.int32)
    sched[c % 7 == 3] = -1
    return sched


def irrigation_rows0(sched):
    """RATE and NLEFT of elmk_irrigation_init: a window of 1 .. 7 steps open already in one irrigated column in three."""
    c = np.arange(NCOL)
    on = (sched >= 0) & (c % 3 == 0)
    return np.where(on, 1.0e-4 + 1.0e-6 * (c % 97), 0.0), np.where(on, 1.0 + c % 7, 0.0)


def network_a(placed):
    """A forest along a random order of the cells (every edge runs forward in that order, so there is no cycle) whose hub, a cell
    late in the order that holds no placed path, takes exactly eight cells: four of lower and four of higher index.  Returns (down,
    hub, the eight sources)."""
    rng = np.random.default_rng(79)
    perm = rng.permutation(NCELL)
    taken = set(placed)
    hub_at = next(k for k in range(58, NCELL) if int(perm[k]) not in taken and 8 < int(perm[k]) < NCELL - 8)
    hub = int(perm[hub_at])
    early = [int(x) for x in perm[:hub_at] if int(x) not in taken]
    srcs = [x for x in early if x < hub][:4] + [x for x in early if x > hub][:4]
    assert len(srcs) == 8
    down = np.full(NCELL, -1, np.int32)
    deg = np.zeros(NCELL, np.int64)
    for i in range(NCELL - 1):
        u = int(perm[i])
        if u in srcs:
            down[u] = hub
            continue
        if rng.random() < 0.1:
            continue
        j = int(perm[rng.integers(i + 1, min(i + 13, NCELL))])
        if j != hub and deg[j] < 8:
            down[u] = j
            deg[j] += 1
    return down, hub, np.array(sorted(srcs))


def _finite(x):
    return np.where(np.isfinite(x) & (np.abs(x) < 1e200), x, 7.0)


@functools.lru_cache(maxsize=None)
def geometry():
    """Everything of the case that lives on cells, and the irrigation's schedule: a dict.  The storages: inundation_cases' placed
    cells hold the thirteen paths of the exchange; the hub of network A stands at 98 % of its channel under eight sources at three
    times theirs, so it crosses its bank within a call; every fourth cell without a place holds a thousandth of what was drawn, which
    puts it under a day's demand."""
    m = sc.cell_map(NCOL, NCELL, 71, empty=(0, 63, 64), single=(5,), free=3)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(NCELL, 78)
    volr0, wh0, wt0 = _finite(volr0), _finite(wh0), _finite(wt0)
    rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(NCELL, 80, area, p0, volr0, wh0, wt0, NSUB_A, DT)
    wf = _finite(wf)
    placed = [c for c, _, _ in ic.placed_cells(NCELL)]
    down_a, hub, srcs = network_a(placed)
    tab = rt.inundation_tables(area, p, rdepth, eprof)
    low = np.array([c for c in range(NCELL) if c % 4 == 2 and c not in placed and c != hub and c not in srcs])
    volr[low] = np.abs(volr[low]) * 1.0e-3
    wf[low] = 0.0
    volr[hub], wf[hub], wh[hub], wt[hub] = 0.98 * tab["VC"][hub], 0.0, 0.0, 0.0
    volr[srcs], wf[srcs] = 3.0 * tab["VC"][srcs], 0.0
    sched = irrigation_sched()
    rate0, nleft0 = irrigation_rows0(sched)
    return dict(map=m, area=area, ddist=ddist, params=p, rdepth=rdepth, eprof=eprof, tab=tab, volr=volr, wh=wh, wt=wt, wf=wf, down_a=down_a,
                down_b=np.append(np.arange(1, NCELL), -1).astype(np.int32), hub=hub, srcs=srcs, low=low, placed=placed, sched=sched,
                rate0=rate0, nleft0=nleft0)


def network(G, which):
    """(down, nsub) of network "A" or "B"."""
    return (G["down_a"], NSUB_A) if which == "A" else (G["down_b"], NSUB_B)


# ---- the state ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case():
    """geometry() and the columns: a dict.  The irrigation's generated tier (thawed, rooted, stressed and unstressed columns), the
    hydrology's prepared rows on it, the permafrost tier on top (frozen layers in twelve columns of thirteen, q_perch_max > 0), a thaw
    front for the active layer in the columns the permafrost tier left thawed, relative humidity in atm_qbot, elevations with longwave
    groups that leave nine columns out, and two aerosol streams."""
    from tests.hydrology_cases import add_frost, clear_snow, prepare
    from tests.irrigation_cases import generated
    from tests.run_cases import _inputs

    G = dict(geometry())
    cols, scal, soil, _ = generated(NCOL, SEED)
    _, _, _, lat, lon, rec = _inputs(NCOL, SEED, nrec=NREC)  # (the same generator call: the records belong to these columns)
    rec = dict(rec)
    rec["atm_qbot"] = np.clip(rec["atm_qbot"] * 5000.0, 5.0, 100.0)  # relative humidity, percent
    clear_snow(cols)
    rows = prepare(cols, SEED + 1)
    frost = add_frost(cols, rows, SEED + 2)
    cols["altmax_indx"] = np.full(NCOL, 5, np.int32)
    cols["altmax_lastyear_indx"] = np.zeros(NCOL, np.int32)
    rng = np.random.default_rng(SEED + 3)
    hf = 200.0 + 1500.0 * rng.random(NCOL)
    hc = hf + rng.uniform(-1500.0, 1500.0, NCOL)
    cell = np.arange(NCOL) // 60
    cell[NCOL - 9:] = -1  # columns in no group
    groups = RG.owner_map(cell, 0.5 + rng.random(NCOL), int(cell.max()) + 1)
    dep = {s: 1.0e-12 * (1.0 + k + rng.random((12, NCOL))) for k, s in enumerate(AEROSOL_STREAMS)}
    G.update(cols=cols, scal=scal, soil=soil, lat=lat, lon=lon, rec=rec, rows=rows, frost=frost, hc=hc, hf=hf, groups=groups, dep=dep,
             altmax0=(0.01 * np.arange(NCOL), 5.0 - 0.02 * np.arange(NCOL)))
    return G


# ---- the context -------------------------------------------------------------------------------------------------------------------
def reserve(D, G, max_steps=NSTEPS):
    """elmk_run_reserve and everything a new reservation forgets: the series and the record times."""
    from tests.run_cases import upload_series

    D.run_reserve(NREC, max_steps)
    upload_series(D, G["rec"])
    D.series_record_times(0, REC_TIMES)


def enable_routing(D, G, which="A", withdraw=True, kinematic=True, flood=True):
    down, nsub = network(G, which)
    D.routing_enable(down, G["ddist"], G["area"], rt.EFFVEL, nsub)
    if withdraw:
        D.routing_set_withdrawal(True)
    if kinematic:
        D.routing_kinematic_enable(G["params"])
    if kinematic and flood:
        D.routing_inundation_enable(G["rdepth"], G["eprof"])


def add_entries(D, families=ROW_FAMILIES, tapes=(0, 1)):
    """The field entries (every op, two tapes), a per-column and a gridded entry over a row of each family of `families`, and the two
    accumulator entries.  The ids are kept on the context: D._hist is [(entry, tape)], D._accum the accumulator ids."""
    D._hist = [(D.history_add(t, f, op), t) for t, f, op in FIELD_ENTRIES]
    add_row_entries(D, families, tapes)
    D._accum = [D.accum_add(*e) for e in ACCUM_ENTRIES]


def add_row_entries(D, families, tapes):
    for i, (fam, which) in enumerate(ROW_ENTRIES):
        if fam in families:
            a, b = tapes[i % 2], tapes[(i + 1) % 2]
            D._hist.append((D.history_add_row(a, fam, which, "avg"), a))
            D._hist.append((D.gridded_history_add_row(b, fam, which, "max"), b))


def full_context(graph, lib_path=None, G=None, thr=THR, withdraw=True, init=True, families=ROW_FAMILIES, poisoned=False):
    """A context with all of it on.  thr None: the river supply limit stays off; withdraw False: and the withdrawal too; init False:
    the prognostic rows beside the state keep their zeros (a restart hands them over); families: the feature families that get history
    entries over a row (a family with an entry cannot be cleared); poisoned: every field a restart image does not hold is NaN."""
    from tests.hydrology_cases import _new_frost
    from tests.run_cases import poison

    G = G or case()
    D = _new_frost(G["cols"], G["scal"], G["soil"], G["rows"], G["frost"], lib_path, G["lat"], G["lon"])
    D.set_graph(graph)
    D.set_shortwave_mode("coszen", FORC_DT)
    reserve(D, G)
    D.set_column_elevation(G["hc"], G["hf"])
    D.set_downscaling_groups(*G["groups"])
    D.set_downscaling("topo")
    D.aerosol_reserve()
    for s in AEROSOL_STREAMS:
        D.aerosol_upload(s, 0, G["dep"][s])
    D.active_layer_enable()
    D.water_balance_enable(TOL)
    D.set_output_grid(*G["map"], fill=NAN)
    D.irrigation_enable(G["sched"])
    enable_routing(D, G, "A", withdraw=withdraw)
    if thr is not None:
        D.irrigation_supply_enable(thr)
    if init:
        D.active_layer_init(*G["altmax0"])
        D.irrigation_init(G["rate0"], G["nleft0"])
        D.routing_init(G["volr"])
        D.routing_kinematic_init(G["wh"], G["wt"])
        D.routing_inundation_init(G["wf"])
    add_entries(D, families)
    if poisoned:
        poison(D)
    return D


# ---- the same steps through the stand-alone calls ------------------------------------------------------------------------------------
def full_stepwise(D, rec, steps, dt=DT):
    """run_cases.stepwise with every stage on and the record times.  What elmk_run keeps in its ring rows is kept on the context
    (D._diag) for full_snapshot."""
    from tests.run_cases import stepwise

    r = stepwise(D, rec, steps, ALL_FLAGS, dt, rec_times=REC_TIMES)
    mms, nbad, first = zip(*r.bal)
    D._diag = tuple(r) + (np.array(mms), np.array(nbad, np.int64), np.array(first, np.int64))


def run(D, steps, flags=ALL_FLAGS, dt=DT):
    """elmk_run; what a stepwise call left on the context for full_snapshot is forgotten."""
    D._diag = None
    D.run(dt, steps, flags)


# ---- everything a step can change --------------------------------------------------------------------------------------------------
def _opt(call):
    """The call's value, or None while the feature it reads is off."""
    try:
        return call()
    except L.ElmkError:
        return None


def full_snapshot(D):
    """Every non-series field; the diagnostics rows and the water balance's triples and census of the last run (of the last stepwise
    call on a context that was stepped); the rows of the active layer, the hydrology, the frost table, the water balance, the
    irrigation and the supply limit; the ten routing rows and the count; every history read with its tape's count; every accumulator
    read with its count.  A part whose feature is off is None."""
    from tests.run_cases import SERIES

    out = {k: D[k] for k in D.fields if k not in SERIES}
    diag = getattr(D, "_diag", None)
    if diag is None:
        diag = tuple(D.run_diagnostics()) + tuple(D.run_water_balance())
    for name, v in zip(("cons", "flags", "first_flagged", "wb_triples", "wb_nbad", "wb_first"), diag):
        out["diag/" + name] = np.asarray(v)
    out["rows/alt"] = _opt(lambda: np.stack([D.active_layer_read(w) for w in range(3)]))
    out["rows/hydrology"] = _opt(D.soil_hydrology_rows)
    out["rows/frost"] = _opt(D.soil_hydrology_frost_rows)
    out["rows/water_balance"] = _opt(D.water_balance_rows)
    out["rows/irrigation"] = _opt(D.irrigation_rows)
    out["rows/supply"] = _opt(lambda: np.stack([D.irrigation_supply_read(w) for w in SUP_ROWS]))
    for w in ROUTE_ROWS:
        out[f"route/{w}"] = _opt(lambda w=w: D.routing_read(w))
    out["route/count"] = _opt(lambda: np.array(D.routing_count()))
    for e, tape in getattr(D, "_hist", ()):
        n = D.history_count(tape)
        out[f"hist/{e}"] = (np.array(n), D.history_read(e) if n > 0 else None)
    for e in getattr(D, "_accum", ()):
        v, n = D.accum_read(e)
        out[f"accum/{e}"] = (np.array(n), v)
    return out


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return same(a, b)


def assert_same_snapshot(got, want, what="", skip=()):
    """Bit for bit in every part."""
    assert got.keys() == want.keys(), (what, sorted(set(got) ^ set(want)))
    differ = [k for k in want if k not in skip and not _same(got[k], want[k])]
    assert not differ, (what, differ[:12], len(differ))
