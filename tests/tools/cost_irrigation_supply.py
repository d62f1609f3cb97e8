#!/usr/bin/env python3
"""GPU box: what the irrigation's river supply limit costs, alone and inside elmk_run.  (The file is not called
irrigation_supply_cost.py because tests/test_cost_tools_host.py pins the number of *_cost.py tools.)

Default mode, per column count, four columns per cell (every column in one cell, weight 1/4), outlet-only cells, 48 longitude bands on
the clock (irrigation_cost.band_sched).  The limiter has no entry point of its own - elmk_irrigation enqueues it behind k_irrigation -
so it is timed as a difference: the same series of 40 calls back to back with the limit off and on, interleaved over `rounds`:
    irr_idle, irr_idle+limit   no column checks (between the bands' clocks): the limiter reads the map, RATE, NLEFT and QFLX_IRRIG
                               once and writes three cell rows; 36 B per column + 64 B per cell = 52 B per column on the tally
    irr_band, irr_band+limit   band 24 (one column in 48) passes 06:00 local and checks; its cells are limited where VOLR is short
    accum_t10                  elmk_accum_update with the single t10 entry (32 B per column): the streaming yardstick of the
                               irrigation's own record; limiter_quiet_over_accum_t10 is a ratio to report, not a bound
--run: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_IRRIGATION | ELMK_RUN_ROUTING (the withdrawal on),
  the limit off against on, the snapshot restored before every run.
--parent LIB: the same flagged step with the limit never enabled, alternated between this build and LIB, a build of the parent commit's
  library (which has every feature but the limit): the limit-off step must not have moved.  --parent2 LIB2: a second build of the
  parent in this build's place, the margin between two builds of one source.  --parent-first: the parent's context is created first.
Prints one JSON line per count (profiles/r21_irrigation_supply_cost.jsonl).
python tests/tools/cost_irrigation_supply.py [--cols 1000000,10000000] [--rounds 5] [--run] [--run-steps 6] [--parent LIB [--parent-first] [--parent2 LIB2]] [--out FILE]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
import irrigation_cost as IC  # noqa: E402
import water_balance_cost as WB  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import routing as rt  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = IC.CALLS
COLS_PER_CELL = 4
THR = 0.1
QUIET_BYTES = 36 + 64 // COLS_PER_CELL  # per column: col 4, w 8, RATE 8, NLEFT 8, QFLX_IRRIG 8; per cell: ptr 8, area 8, VOLR 8, UNMET_SUM 16, three rows 24
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_IRRIGATION | st.RUN_ROUTING
RUN = CL.arg("--run", action="store_true")


def build(cols, lib_path=None):
    """The water balance's context with an output grid of four columns per cell, outlet-only routing with the withdrawal on and the
    irrigation on the 48 bands' clocks; the limit is not enabled."""
    D = WB.build(cols, lib_path=lib_path)
    ncells = cols // COLS_PER_CELL
    n = ncells * COLS_PER_CELL
    D.set_output_grid(np.arange(ncells + 1, dtype=np.int64) * COLS_PER_CELL, np.arange(n, dtype=np.int32), np.full(n, 1.0 / COLS_PER_CELL))
    rng = np.random.default_rng(3)
    D.routing_enable(np.full(ncells, -1, np.int32), np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), ncells)), np.full(ncells, 1.0e8),
                     rt.EFFVEL, 1)
    D._volr = rng.uniform(0.0, 1.0e6, ncells)
    D.routing_init(D._volr)
    D.irrigation_enable(IC.band_sched(cols))
    D.routing_set_withdrawal(True)
    return D


def measure(cols, rounds):
    D = build(cols)
    accum.add_t10(D, DT)
    sched = IC.band_sched(cols)
    tod_band = (21600 - 24 * 1800) % 86400
    idle_tod = IC.NOON + 900
    assert not (((idle_tod + sched.astype(np.int64)) % 86400 - 21600) % 86400 < IC.IDLE_DT).any()
    launches = {"irr_idle": lambda: D.irrigation(IC.IDLE_DT, idle_tod), "irr_band": lambda: D.irrigation(DT, tod_band)}
    res = {m: [] for m in ("irr_idle", "irr_idle+limit", "irr_band", "irr_band+limit", "accum_t10")}
    limited = []
    for r in range(rounds):
        for limit in CL.interleave(r, (False, True)):
            if limit:
                D.irrigation_supply_enable(THR)
            for mode in CL.interleave(r, ("irr_idle", "irr_band")):
                D.irrigation_init()
                D.routing_init(D._volr)
                res[mode + ("+limit" if limit else "")].append(CL.back_to_back(D, launches[mode], CALLS))
                if limit and mode == "irr_band":
                    limited.append(int((D.irrigation_supply_read(st.IRRSUP_RATIO) < 1.0).sum()))
            if limit:
                D.irrigation_supply_clear()
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
    med = CL.medians(res)
    D.close()
    quiet, band = med["irr_idle+limit"] - med["irr_idle"], med["irr_band+limit"] - med["irr_band"]
    return {"columns": cols, "cells": cols // COLS_PER_CELL, "rounds": rounds, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "limiter_quiet_ms": quiet, "limiter_band_ms": band, "limited_cells_per_round": limited,
            "limiter_quiet_bytes": QUIET_BYTES * cols, "limiter_quiet_GBps": QUIET_BYTES * cols / (quiet * 1e-3) / 1e9 if quiet > 0 else None,
            "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9, "limiter_quiet_over_accum_t10": quiet / med["accum_t10"]}


def measure_run(cols, rounds, run_steps):
    D = build(cols)
    steps = CL.schedule(run_steps)
    res = {"run": [], "run+limit": []}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            if key == "run+limit":
                D.irrigation_supply_enable(THR)
            D.soil_hydrology_init()
            D.irrigation_init()
            D.routing_init(D._volr)
            res[key].append(CL.run_ms(D, steps, FLAGS))
            if key == "run+limit":
                D.irrigation_supply_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // COLS_PER_CELL, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_with_over_without": med["run+limit"] / med["run"],
            "run_step_added_ms": med["run+limit"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent's library has no elmk_irrigation_supply_*: neither context enables the limit, both run the flagged step."""
    steps = CL.schedule(run_steps)

    def time_one(D):
        D.soil_hydrology_init()
        D.irrigation_init()
        D.routing_init(D._volr)
        return CL.run_ms(D, steps, FLAGS)

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], lambda n, p: build(n, lib_path=p), time_one,
                             first="parent" if parent_first else "this", optional=("elmk_irrigation_supply",), baseline="parent")
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "run_ms_all": c["all"], "run_ms_median": c["median"], "spread": c["spread"], "this_over_parent": c["this_over_parent"]}


def main():
    a = CL.cli("1000000,10000000", 5, (RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
