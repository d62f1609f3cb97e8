#!/usr/bin/env python3
"""GPU box: what the runoff routing costs, alone and inside elmk_run.  (The file is not called routing_cost.py because
tests/test_cost_tools_host.py pins the number of *_cost.py tools.)

--cells N1,N2,N3 (default mode): per cell count, one cell per column, every cell's column its own (weight 1), a network in which every
  cell of an nlon-wide grid drains into one of its four southern / eastern neighbours (in-degree <= 4) and the last row is outlets.
  Interleaved over `rounds` repeats:
    call_nsub1  elmk_routing with nsub = 1: two launches (R1, one sub-step), 40 calls back to back
    call_nsub8  the same with nsub = 8: nine launches
  Byte tally per cell: R1 reads 8 (ptr) + 4 (col) + 8 (w) + 8 (QRUNOFF) + 8 (area) and writes 8 (+ 16 for the copy of an odd nsub); a
  sub-step reads 24 + 4 npad (map) + 16 per upstream cell (+ 8 past the first) and writes 16 (+ 16 in the last).
--run: per column count (--cols), four columns per cell, the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE against the same
  with ELMK_RUN_ROUTING (nsub = 4), the snapshot restored before every run.
--parent LIB: the unflagged run step (ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE, routing never enabled) alternated between this
  build and LIB, a build of the parent commit's library: the unflagged step must not have moved.  --parent2 LIB2: a second build of
  the parent in this build's place, the margin between two builds of one source.
Prints one JSON line per count (profiles/r19_routing_cost.jsonl).
python tests/tools/cost_routing.py [--cols 10000,200000,4000000] [--rounds 5] [--run] [--run-steps 6] [--parent LIB [--parent-first] [--parent2 LIB2]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
import water_balance_cost as WB  # noqa: E402
from elmkernels_amd import routing as rt  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = 40  # calls of a back-to-back series
UNFLAGGED = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE
RUN = CL.arg("--run", action="store_true")


def network(ncells, seed=7):
    """Every cell of an nlon-wide grid drains east, south-west, south or south-east; the last row drains nowhere."""
    nlon = max(2, int(np.sqrt(ncells)))
    rng = np.random.default_rng(seed)
    c = np.arange(ncells, dtype=np.int64)
    d = c + np.array([1, nlon - 1, nlon, nlon + 1])[rng.integers(0, 4, ncells)]
    return np.where(d < ncells, d, -1).astype(np.int32)


def build(cols, lib_path=None, per_cell=1, nsub=None):
    D = WB.build(cols, lib_path=lib_path)
    ncells = cols // per_cell
    D.set_output_grid(np.arange(ncells + 1, dtype=np.int64) * per_cell, np.arange(ncells * per_cell, dtype=np.int32),
                      np.full(ncells * per_cell, 1.0 / per_cell))
    if nsub:
        rng = np.random.default_rng(3)
        D.routing_enable(network(ncells), np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), ncells)), np.full(ncells, 1.0e8), rt.EFFVEL, nsub)
        D.routing_init(rng.uniform(0.0, 1.0e6, ncells))
    return D


def measure(cells, rounds):
    D = build(cells)
    down = network(cells)
    npad = rt.npad_of(rt.upstream_map(down))
    rng = np.random.default_rng(3)
    ddist, volr = np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), cells)), rng.uniform(0.0, 1.0e6, cells)
    D.water_balance_begin()
    D.water_balance(DT)
    res = {"call_nsub1": [], "call_nsub8": []}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.routing_enable(down, ddist, np.full(cells, 1.0e8), rt.EFFVEL, 1 if key == "call_nsub1" else 8)
            D.routing_init(volr)
            res[key].append(CL.back_to_back(D, lambda: D.routing(DT), CALLS))
            D.routing_clear()
    med = CL.medians(res)
    D.close()
    ups = float((down >= 0).sum()) / cells
    step_bytes = 24 + 4 * npad + 16 * ups + 16
    return {"cells": cells, "rounds": rounds, "npad": npad, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "launches": {"call_nsub1": 2, "call_nsub8": 9}, "ms_per_launch": {"call_nsub1": med["call_nsub1"] / 2, "call_nsub8": med["call_nsub8"] / 9},
            "bytes_per_cell": {"r1": 44 + 16, "sub_step": step_bytes}}


def measure_run(cols, rounds, run_steps):
    D = build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    res = {"run": [], "run+routing": []}
    for r in range(rounds):
        for key, flags in CL.interleave(r, (("run", UNFLAGGED), ("run+routing", UNFLAGGED | st.RUN_ROUTING))):
            D.soil_hydrology_init()
            res[key].append(CL.run_ms(D, steps, flags))
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_with_over_without": med["run+routing"] / med["run"],
            "run_step_added_ms": med["run+routing"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent's library has no elmk_routing_*: neither context enables the feature, both run the unflagged step."""
    steps = CL.schedule(run_steps)

    def time_one(D):
        D.soil_hydrology_init()
        return CL.run_ms(D, steps, UNFLAGGED)

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], lambda n, p: WB.build(n, lib_path=p), time_one,
                             first="parent" if parent_first else "this", optional=("elmk_routing",), baseline="parent")
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "run_ms_all": c["all"], "run_ms_median": c["median"], "spread": c["spread"], "this_over_parent": c["this_over_parent"]}


def main():
    a = CL.cli("10000,200000,4000000", 5, (RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
