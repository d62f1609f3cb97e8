#!/usr/bin/env python3
"""GPU box: what the stream temperature costs beside the kinematic-wave scheme it extends, alone and inside elmk_run.  A tool of its own
on cost_routing.py's network and contexts and cost_routing_kinematic.py's parameters; those tools and their records stay what they are.
(Not called *_cost.py: tests/test_cost_tools_host.py pins the number of those.)

default mode (--cols N1,N2 are cell counts): per count, one cell per column, cost_routing's network.  Interleaved over `rounds` repeats,
  in one process, 40 calls back to back each, nsub = 1 (two launches) and 8 (nine launches):
    kw_nsub*          elmk_routing with the kinematic-wave scheme, the extension off
    heat_nsub*        the HEAT form
  and the ratios over kw; a middle sub-step is (nsub8 - nsub1) / 7.  Byte tally per cell of a middle sub-step:
  the kinematic sub-step streams 176; the HEAT form reads TT, TR, hr, H1's eight rows and the four running diagnostics, 120, and writes
  TT, TR, the four diagnostics and hr, 56: 352, and 8 more per upstream slot gathered.  The record gives both forms' TB/s on their
  tallies: a HEAT sub-step at the plain form's rate is stream-bound like it, one below it is bound by the issue of its two exp and
  four divisions.
--run: per column count, four columns per cell, nsub = 4: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE |
  ELMK_RUN_ROUTING under the kinematic scheme against the same with the extension on, the snapshot restored before every run.
--parent LIB: the kinematic call with the extension off (--nsub sub-steps, one cell per column) alternated between this build and LIB, a
  build of the parent commit's library, two contexts of one process taking turns.  --parent-first: the parent's context is created
  first.  --parent2 LIB2: a second copy of the parent in this build's place, the spread two copies of one source show.
Prints one JSON line per count (profiles/r25_routing_heat_cost.jsonl).
python tests/tools/cost_routing_heat.py [--cols 200000,4000000] [--rounds 5] [--run] [--run-steps 6]
                                        [--parent LIB [--nsub 8] [--parent-first] [--parent2 LIB2]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_routing as CR  # noqa: E402
import cost_routing_kinematic as CK  # noqa: E402
import costlib as CL  # noqa: E402
from elmkernels_amd import routing as rt  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = CR.CALLS
KW_SUB_STEP_BYTES = 176
HEAT_SUB_STEP_BYTES = KW_SUB_STEP_BYTES + 120 + 56


def heat_on(D, ncells):
    """The extension with half the cells half shaded, water of 285 K."""
    D.routing_heat_enable(2, np.where(np.arange(ncells) % 2 == 0, 0.5, 0.0))
    D.routing_heat_init(np.full(ncells, 285.0), np.full(ncells, 285.0))


def measure(cells, rounds):
    down = CR.network(cells)
    up = rt.upstream_map(down)
    npad, slots = rt.npad_of(up), float((up >= 0).sum()) / cells
    rng = np.random.default_rng(3)
    ddist, volr = np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), cells)), rng.uniform(0.0, 1.0e6, cells)
    D = CR.build(cells)
    D.water_balance_begin()
    D.water_balance(DT)
    res = {f"{t}_nsub{n}": [] for n in (1, 8) for t in ("kw", "heat")}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            tier, nsub = key.split("_nsub")
            D.routing_enable(down, ddist, np.full(cells, 1.0e8), rt.EFFVEL, int(nsub))
            D.routing_init(volr)
            CK.kw_on(D, cells)
            if tier == "heat":
                heat_on(D, cells)
            res[key].append(CL.back_to_back(D, lambda: D.routing(DT), CALLS))
            D.routing_clear()
    med = CL.medians(res)
    D.close()
    sub = {t: (med[f"{t}_nsub8"] - med[f"{t}_nsub1"]) / 7 for t in ("kw", "heat")}
    bytes_ = {"kw": KW_SUB_STEP_BYTES, "heat": HEAT_SUB_STEP_BYTES, "heat_with_gathers": HEAT_SUB_STEP_BYTES + 8 * slots}
    return {"cells": cells, "rounds": rounds, "npad": npad, "upstream_slots_per_cell": slots, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "launches": {"nsub1": 2, "nsub8": 9}, "sub_step_ms": sub, "bytes_per_cell_sub_step": bytes_,
            "sub_step_TB_per_s": {t: bytes_[t] * cells / (sub[t] * 1.0e-3) / 1.0e12 for t in ("kw", "heat")},
            "over_kw": {f"heat_nsub{n}": med[f"heat_nsub{n}"] / med[f"kw_nsub{n}"] for n in (1, 8)},
            "sub_step_heat_over_kw": sub["heat"] / sub["kw"]}


def measure_run(cols, rounds, run_steps):
    D = CR.build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    flags = CR.UNFLAGGED | st.RUN_ROUTING
    res = {"run+kinematic": [], "run+heat": []}
    CK.kw_on(D, cols // 4)
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.soil_hydrology_init()
            if key == "run+heat":
                heat_on(D, cols // 4)
            res[key].append(CL.run_ms(D, steps, flags))
            if key == "run+heat":
                D.routing_heat_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_heat_over_kinematic": med["run+heat"] / med["run+kinematic"],
            "run_step_heat_added_ms": med["run+heat"] - med["run+kinematic"],
            "bytes_per_cell_sub_step": {"kw": KW_SUB_STEP_BYTES, "heat": HEAT_SUB_STEP_BYTES}}


NSUB = CL.arg("--nsub", type=int, default=4)


def parent_kinematic(cols, rounds, nsub, lib_parent, parent_first, lib_this=None):
    """The parent has the kinematic scheme and not the extension: both contexts turn the scheme on and take turns at its call."""
    def build(n, p):
        D = CR.build(n, lib_path=p, nsub=nsub)
        CK.kw_on(D, n)
        D.water_balance_begin()
        D.water_balance(DT)
        return D

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], build,
                             {"kinematic_call": lambda D: CL.back_to_back(D, lambda: D.routing(DT), CALLS)},
                             first="parent" if parent_first else "this", optional=("elmk_routing_heat",))
    return {"cells": cols, "nsub": nsub, "rounds": rounds, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"], "bytes_per_cell_sub_step": KW_SUB_STEP_BYTES,
            "kinematic_call_this_over_parent": c["median"]["this"]["kinematic_call"] / c["median"]["parent"]["kinematic_call"]}


def main():
    a = CL.cli("200000,4000000", 5, (CR.RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2, NSUB), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent_kinematic(c, a.rounds, a.nsub, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
