#!/usr/bin/env python3
"""GPU box: what the kinematic-wave routing costs beside the linear scheme, alone and inside elmk_run.  A tool of its own beside
cost_routing.py, whose network, contexts and constants it takes: that tool and its records (profiles/r19_routing_cost.jsonl) stay what
they are.  (Not called *_cost.py: tests/test_cost_tools_host.py pins the number of those.)

default mode (--cols N1,N2,N3 are cell counts): per count, one cell per column, cost_routing's network (in-degree <= 4).  Interleaved over
  `rounds` repeats, both schemes on the same network in the same process, 40 calls back to back each:
    call_nsub1 / call_nsub8  elmk_routing with the linear scheme, nsub = 1 (two launches) and 8 (nine launches)
    kw_nsub1 / kw_nsub8      the same with the kinematic-wave scheme on (the same launch counts)
  and the ratios kinematic over linear.  Byte tally per cell of a middle kinematic sub-step (neither first nor last): fifteen 8-byte
  rows read (WH, WT, VOLR, the cell's own er, area, QSUR, QSUB, the running QOUT and the seven parameter rows: CH, TLEN, TWIDTH, CT for
  eh and et, RLEN, RWIDTH, CR for the er of the new VOLR), 4 npad of map and five rows written (WH, WT, VOLR, QOUT, er) are streamed:
  160 + 4 npad; the gathers add at most 8 per upstream slot, fewer where neighbours share lines.  Arithmetic: three pow and ten
  divisions.
--run: per column count, four columns per cell, nsub = 4: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE against the
  same with ELMK_RUN_ROUTING under the linear scheme and under the kinematic one, the snapshot restored before every run.
--parent LIB: with the routing enabled in both contexts (the parent has the linear scheme) and the kinematic scheme in neither, the
  unflagged run step and the linear call (nsub = 4, four columns per cell) alternated between this build and LIB, a build of the parent
  commit's library.  --parent2 LIB2: a second build of the parent in this build's place, the margin between two builds of one source.
Prints one JSON line per count (profiles/r20_routing_kinematic_cost.jsonl).
python tests/tools/cost_routing_kinematic.py [--cols 10000,200000,4000000] [--rounds 5] [--run] [--run-steps 6]
                                             [--parent LIB [--parent-first] [--parent2 LIB2]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_routing as CR  # noqa: E402
import costlib as CL  # noqa: E402
from elmkernels_amd import routing as rt  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = CR.CALLS
UNFLAGGED = CR.UNFLAGGED
KW_BASE = (0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04)  # HSLP .. NR of a mid-sized cell


def kw_params(ncells, seed=5):
    """Every parameter within a factor of two of a mid-sized cell's."""
    return np.array(KW_BASE)[:, None] * np.exp(np.random.default_rng(seed).uniform(np.log(0.5), np.log(2.0), (rt.NPARAM, ncells)))


def kw_on(D, ncells, seed=3):
    rng = np.random.default_rng(seed)
    D.routing_kinematic_enable(kw_params(ncells))
    D.routing_kinematic_init(rng.uniform(0.0, 1.0e6, ncells), rng.uniform(0.0, 1.0e6, ncells))


def measure(cells, rounds):
    D = CR.build(cells)
    down = CR.network(cells)
    npad = rt.npad_of(rt.upstream_map(down))
    rng = np.random.default_rng(3)
    ddist, volr = np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), cells)), rng.uniform(0.0, 1.0e6, cells)
    D.water_balance_begin()
    D.water_balance(DT)
    res = {"call_nsub1": [], "call_nsub8": [], "kw_nsub1": [], "kw_nsub8": []}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.routing_enable(down, ddist, np.full(cells, 1.0e8), rt.EFFVEL, 1 if key.endswith("nsub1") else 8)
            D.routing_init(volr)
            if key.startswith("kw"):
                kw_on(D, cells)
            res[key].append(CL.back_to_back(D, lambda: D.routing(DT), CALLS))
            D.routing_clear()
    med = CL.medians(res)
    D.close()
    ups = float((down >= 0).sum()) / cells
    # a middle sub-step (neither first nor last): what it streams, what its gathers add at the most, and the rates those bytes make
    kw_streamed, kw_gathered = 8 * 15 + 4 * npad + 8 * 5, 8 * npad
    sub_ms = (med["kw_nsub8"] - med["kw_nsub1"]) / 7
    rate = lambda b: b * cells / (sub_ms * 1e-3) / 1e9 if sub_ms > 0 else None  # noqa: E731
    return {"cells": cells, "rounds": rounds, "npad": npad, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "launches": {"nsub1": 2, "nsub8": 9}, "bytes_per_cell": {"linear_sub_step": 24 + 4 * npad + 16 * ups + 16, "kw_sub_step_streamed": kw_streamed,
                                                                 "kw_sub_step_gathered_at_most": kw_gathered},
            "kinematic_over_linear": {"nsub1": med["kw_nsub1"] / med["call_nsub1"], "nsub8": med["kw_nsub8"] / med["call_nsub8"]},
            "kw_sub_step_ms": sub_ms, "kw_sub_step_gb_per_s": {"streamed": rate(kw_streamed), "with_every_gather": rate(kw_streamed + kw_gathered)},
            "linear_sub_step_ms": (med["call_nsub8"] - med["call_nsub1"]) / 7}


def measure_run(cols, rounds, run_steps):
    D = CR.build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    modes = (("run", UNFLAGGED), ("run+routing", UNFLAGGED | st.RUN_ROUTING), ("run+kinematic", UNFLAGGED | st.RUN_ROUTING))
    res = {key: [] for key, _ in modes}
    for r in range(rounds):
        for key, flags in CL.interleave(r, modes):
            D.soil_hydrology_init()
            if key == "run+kinematic":
                kw_on(D, cols // 4)
            res[key].append(CL.run_ms(D, steps, flags))
            if key == "run+kinematic":
                D.routing_kinematic_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_linear_over_without": med["run+routing"] / med["run"],
            "run_step_linear_added_ms": med["run+routing"] - med["run"], "run_step_kinematic_over_without": med["run+kinematic"] / med["run"],
            "run_step_kinematic_added_ms": med["run+kinematic"] - med["run"]}


def parent_linear(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent has the linear scheme: both contexts enable the routing and neither the kinematic scheme; the unflagged step and the
    linear call take turns."""
    steps = CL.schedule(run_steps)

    def step(D):
        D.soil_hydrology_init()
        return CL.run_ms(D, steps, UNFLAGGED)

    def call(D):
        return CL.back_to_back(D, lambda: D.routing(DT), CALLS)

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], lambda n, p: CR.build(n, lib_path=p, per_cell=4, nsub=4),
                             {"unflagged_step": step, "linear_call": call}, first="parent" if parent_first else "this",
                             optional=("elmk_routing_kinematic",))
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"],
            "linear_this_over_parent": {m: c["median"]["this"][m] / c["median"]["parent"][m] for m in ("unflagged_step", "linear_call")}}


def main():
    a = CL.cli("10000,200000,4000000", 5, (CR.RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent_linear(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
