#!/usr/bin/env python3
"""GPU box: what cell rows on history tapes cost (elmk_cell_history_add_row; k_hist_accumulate_rows), and that a context without them
pays nothing.  The context is cost_irrigation_supply.py's: four columns per cell, outlet-only routing.

Default mode, per cell count: elmk_history_accumulate, 40 calls back to back, with 1, 4 and 10 cell-row entries and nothing else on the
tapes (rows VOLR, QIN, QOUT, QOUT_SUM in turn, ops AVG, MAX, MIN, SUM, INST in turn), interleaved over `rounds`:
    cellrows_K   ms per launch, and TB/s on 24 B per cell and row (8 B source, 16 B accumulator read and written)
    accum_t10    elmk_accum_update with the single t10 entry (32 B per column): the streaming yardstick of the other records
--parent LIB: a context WITHOUT cell-row entries - a t_grnd AVG entry and a gridded t_grnd entry, so the launch is
  k_hist_accumulate_cells in both - timed on this build and on LIB, a build of the parent commit's library: the accumulate launch and
  the flagged run step (ELMK_RUN_HISTORY | HYDROLOGY | WATER_BALANCE | IRRIGATION | ROUTING), alternated.  --parent2 LIB2: a second
  copy of the parent in this build's place, the spread between two copies of one source.  --parent-first: the parent's context first.
Prints one JSON line per count (profiles/r23_cell_history_cost.jsonl).
python tests/tools/cost_cell_history.py [--cols 16000000] [--rounds 5] [--run-steps 6] [--parent LIB [--parent-first] [--parent2 LIB2]] [--out FILE]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_irrigation_supply as CS  # noqa: E402
import costlib as CL  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = 40
ROWS = (st.ROUTE_VOLR, st.ROUTE_QIN, st.ROUTE_QOUT, st.ROUTE_QOUT_SUM)
OPS = ("avg", "max", "min", "sum", "inst")
COUNTS = (1, 4, 10)
ROW_BYTES = 24  # per cell and row
FLAGS = CS.FLAGS | st.RUN_HISTORY


def measure(cols, rounds):
    D = CS.build(cols)
    ncells = cols // CS.COLS_PER_CELL
    accum.add_t10(D, DT)
    res = {f"cellrows_{k}": [] for k in COUNTS}
    res["accum_t10"] = []
    for r in range(rounds):
        for k in CL.interleave(r, COUNTS):
            for i in range(k):
                D.cell_history_add_row(i % 2, "routing", ROWS[i % len(ROWS)], OPS[i % len(OPS)])
            res[f"cellrows_{k}"].append(CL.back_to_back(D, D.history_accumulate, CALLS))
            D.history_clear()
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": ncells, "rounds": rounds, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "cellrows_TBps": {k: ROW_BYTES * ncells * k / (med[f"cellrows_{k}"] * 1e-3) / 1e12 for k in COUNTS},
            "accum_t10_TBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e12}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """Neither context has a cell-row entry (the parent's library has no such call)."""
    steps = CL.schedule(run_steps)

    def build(n, p):
        D = CS.build(n, lib_path=p)
        D.history_add(0, "t_grnd", "avg")
        D.gridded_history_add(1, "t_grnd", "max")
        return D

    def run_one(D):
        D.soil_hydrology_init()
        D.irrigation_init()
        D.routing_init(D._volr)
        return CL.run_ms(D, steps, FLAGS)

    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
           "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this"}
    modes = {"accumulate": lambda D: CL.back_to_back(D, D.history_accumulate, CALLS), "run_step": run_one}
    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], build, modes,
                             first="parent" if parent_first else "this", optional=("elmk_cell_history_add_row",))
    out.update(ms_all=c["all"], ms_median=c["median"], spread=c["spread"],
               this_over_parent={m: c["median"]["this"][m] / c["median"]["parent"][m] for m in modes})
    return out


def main():
    a = CL.cli("16000000", 5, (CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
