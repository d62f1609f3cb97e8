#!/usr/bin/env python3
"""GPU box: what a record of the point series costs (elmk_points_record; k_points_record), what an armed run step pays for it, and that
a context that never arms it pays nothing.  The context is costlib's run context with an output grid of four columns per cell.

Default mode, per column count: the record launch, 40 calls back to back, at three loads, interleaved over `rounds`:
    gather_8x64      8 entries (levels of t_soisno) at 64 columns: 512 samples
    gather_64x4096   64 entries at 4096 columns: 262144 samples, the largest record (2 MiB)
    gridded_8x64     8 gridded entries at 64 cells of four columns: 512 waves, 2048 terms
  beside, in the same session,
    accum_t10        elmk_accum_update with the single t10 entry (32 B per column): the streaming yardstick of the other records
    hist_1           elmk_history_accumulate with one t_grnd entry (24 B per column)
  and the run step (--run-steps steps, costlib.run_ms) of the same context unarmed and armed with the gather_8x64 load:
    run_unarmed, run_armed   ms per step
--parent LIB: the unarmed run step of this build against LIB, a build of the parent commit's library, alternated (costlib.compare_libraries);
  --parent2 LIB2: a second copy of the parent in this build's place, the spread between two copies of one source; --parent-first: the
  parent's context is created first.  The claim is only that this_over_parent lies inside what two parent copies show.
Prints one JSON line per count (profiles/r27_points_cost.jsonl).
python tests/tools/cost_points.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--parent LIB [--parent-first] [--parent2 LIB2]] [--out FILE]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import regrid  # noqa: E402

DT = CL.DT
CALLS = 40
COLS_PER_CELL = 4
LOADS = ("gather_8x64", "gather_64x4096", "gridded_8x64")


def build(cols, lib_path=None):
    D = CL.run_context(cols, lib_path=lib_path)
    ncells = cols // COLS_PER_CELL
    D.set_output_grid(*regrid.owner_map(np.arange(cols) // COLS_PER_CELL, np.ones(cols), ncells), fill=0.0)
    D.snapshot_fields(list(D.fields))
    return D


def arm(D, load, cols):
    """The entries and lists of one load, 64 records reserved."""
    rng = np.random.default_rng(7)
    nent, npts = (64, 4096) if load == "gather_64x4096" else (8, 64)
    if load.startswith("gridded"):
        D.points_set("cells", rng.integers(0, cols // COLS_PER_CELL, npts))
        for k in range(nent):
            D.points_add_gridded_field("t_soisno", k)
    else:
        D.points_set("columns", rng.integers(0, cols, npts))
        for k in range(nent):
            D.points_add_field("t_soisno", k % 20)
    D.points_reserve(64)


def measure(cols, rounds, run_steps):
    D = build(cols)
    accum.add_t10(D, DT)
    D.history_add(0, "t_grnd", "avg")
    steps = CL.schedule(run_steps)
    res = {k: [] for k in LOADS + ("accum_t10", "hist_1", "run_unarmed", "run_armed")}
    for r in range(rounds):
        for load in CL.interleave(r, LOADS):
            arm(D, load, cols)
            res[load].append(CL.back_to_back(D, lambda: D.points_record(1.0), CALLS))
            D.points_clear()
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
        res["hist_1"].append(CL.back_to_back(D, D.history_accumulate, CALLS))
        for mode in CL.interleave(r, ("run_unarmed", "run_armed")):
            if mode == "run_armed":
                arm(D, LOADS[0], cols)
                D.points_set_run(True)
            res[mode].append(CL.run_ms(D, steps, 0))
            D.points_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // COLS_PER_CELL, "rounds": rounds, "calls": CALLS, "run_steps": run_steps, "ms_median": med,
            "ms_all": res, "spread": CL.spreads(res), "armed_over_unarmed": med["run_armed"] / med["run_unarmed"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """Neither context has the part (the parent's library has no such call): the run step as every context ran it."""
    steps = CL.schedule(run_steps)
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
           "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this"}
    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], build, lambda D: CL.run_ms(D, steps, 0),
                             first="parent" if parent_first else "this", optional=("elmk_points_",), baseline="parent")
    out.update(ms_all=c["all"], ms_median=c["median"], spread=c["spread"], this_over_parent=c["this_over_parent"])
    return out


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds, a.run_steps))


if __name__ == "__main__":
    main()
