#!/usr/bin/env python3
"""GPU box: what the reservoirs cost beside the kinematic-wave scheme they extend, alone and inside elmk_run.  A tool of its own on
cost_routing.py's network and contexts and cost_routing_kinematic.py's parameters; those tools and their records stay what they are.
(Not called *_cost.py: tests/test_cost_tools_host.py pins the number of those.)

default mode (--cols N1,N2 are cell counts): per count, one cell per column, cost_routing's network.  Interleaved over `rounds` repeats,
  in one process, 40 calls back to back each, nsub = 1 (two launches) and 8 (nine launches):
    kw_nsub*          elmk_routing with the kinematic-wave scheme, the extension off
    none_nsub*        the DAM form with no dams (cap = 0 everywhere)
    fiftieth_nsub*    a dam in every fiftieth cell (2 %)
    all_nsub*         a dam in every cell
  and the ratios over kw.  Byte tally per cell of a middle sub-step on top of the kinematic sub-step's 176: every cell of the DAM form
  reads CAP, 8; a dam cell reads its natural er, SMIN, BETA, TARGET[m], KRLS and RES and writes RES and the natural er, 64 more (with
  --reeval-lib, D4's other choice: no natural er row, 48 more and a second K4).
--reeval-lib LIB: the same three DAM tiers on LIB, a build with -DELMK_DAM_REEVAL, beside this build's: D4's two choices.
--run: per column count, four columns per cell, nsub = 4: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE |
  ELMK_RUN_ROUTING under the kinematic scheme against the same with the extension on, a dam in every fiftieth cell, the snapshot
  restored before every run.
--parent LIB: the kinematic call with the extension off (--nsub sub-steps, one cell per column) alternated between this build and LIB, a
  build of the parent commit's library, two contexts of one process taking turns.  --parent-first: the parent's context is created
  first.  --parent2 LIB2: a second copy of the parent in this build's place, the spread two copies of one source show.
Prints one JSON line per count (profiles/r24_routing_reservoir_cost.jsonl).
python tests/tools/cost_routing_reservoir.py [--cols 200000,4000000] [--rounds 5] [--reeval-lib LIB] [--run] [--run-steps 6]
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
TIERS = ("none", "fiftieth", "all")
SHARE = {"none": 0.0, "fiftieth": 0.02, "all": 1.0}
KW_SUB_STEP_BYTES = 176


def dams_on(D, ncells, tier):
    """Dams of 1e9 m3, half full, a target of 20 m3/s and BETA 0.5, in the tier's cells."""
    dam = {"none": np.zeros(ncells, bool), "fiftieth": np.arange(ncells) % 50 == 0, "all": np.ones(ncells, bool)}[tier]
    cap = np.where(dam, 1.0e9, 0.0)
    D.routing_reservoir_enable(cap, np.full((12, ncells), 20.0), np.full(ncells, 0.5), np.zeros(ncells, np.int32))
    D.routing_reservoir_init(0.5 * cap)
    D.routing_reservoir_time(3, False)


def measure(cells, rounds, reeval_lib):
    libs = {"": None}
    if reeval_lib:
        libs["reeval_"] = reeval_lib
    down = CR.network(cells)
    npad = rt.npad_of(rt.upstream_map(down))
    rng = np.random.default_rng(3)
    ddist, volr = np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), cells)), rng.uniform(0.0, 1.0e6, cells)
    ctx = {}
    for tag, lib in libs.items():
        if lib:
            CL.load_build(lib)
        ctx[tag] = CR.build(cells, lib_path=lib)
        ctx[tag].water_balance_begin()
        ctx[tag].water_balance(DT)
    res = {f"{tag}{t}_nsub{n}": [] for n in (1, 8) for tag in libs for t in (("kw",) if not tag else ()) + TIERS}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            tag = "reeval_" if key.startswith("reeval_") else ""
            tier, nsub = key[len(tag):].split("_nsub")
            D = ctx[tag]
            D.routing_enable(down, ddist, np.full(cells, 1.0e8), rt.EFFVEL, int(nsub))
            D.routing_init(volr)
            CK.kw_on(D, cells)
            if tier != "kw":
                dams_on(D, cells, tier)
            res[key].append(CL.back_to_back(D, lambda: D.routing(DT), CALLS))
            D.routing_clear()
    med = CL.medians(res)
    for D in ctx.values():
        D.close()
    tiers = [k[:-len("_nsub1")] for k in res if k.endswith("_nsub1")]
    sub = {t: (med[f"{t}_nsub8"] - med[f"{t}_nsub1"]) / 7 for t in tiers}
    bytes_ = {"kw": KW_SUB_STEP_BYTES}
    for t in TIERS:
        bytes_[t] = KW_SUB_STEP_BYTES + 8 + SHARE[t] * 64
        if reeval_lib:
            bytes_["reeval_" + t] = KW_SUB_STEP_BYTES + 8 + SHARE[t] * 48
    return {"cells": cells, "rounds": rounds, "npad": npad, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "launches": {"nsub1": 2, "nsub8": 9}, "sub_step_ms": sub, "bytes_per_cell_sub_step": bytes_,
            "over_kw": {f"{t}_nsub{n}": med[f"{t}_nsub{n}"] / med[f"kw_nsub{n}"] for n in (1, 8) for t in tiers if t != "kw"}}


def measure_run(cols, rounds, run_steps):
    D = CR.build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    flags = CR.UNFLAGGED | st.RUN_ROUTING
    res = {"run+kinematic": [], "run+dams": []}
    CK.kw_on(D, cols // 4)
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.soil_hydrology_init()
            if key == "run+dams":
                dams_on(D, cols // 4, "fiftieth")
            res[key].append(CL.run_ms(D, steps, flags))
            if key == "run+dams":
                D.routing_reservoir_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_dams_over_kinematic": med["run+dams"] / med["run+kinematic"],
            "run_step_dams_added_ms": med["run+dams"] - med["run+kinematic"],
            "bytes_per_cell_sub_step": {"kw": KW_SUB_STEP_BYTES, "dams": KW_SUB_STEP_BYTES + 8 + 0.02 * 64}}


NSUB = CL.arg("--nsub", type=int, default=4)
REEVAL = CL.arg("--reeval-lib", default=None)


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
                             first="parent" if parent_first else "this", optional=("elmk_routing_reservoir",))
    return {"cells": cols, "nsub": nsub, "rounds": rounds, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"], "bytes_per_cell_sub_step": KW_SUB_STEP_BYTES,
            "kinematic_call_this_over_parent": c["median"]["this"]["kinematic_call"] / c["median"]["parent"]["kinematic_call"]}


def main():
    a = CL.cli("200000,4000000", 5, (CR.RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2, NSUB, REEVAL), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent_kinematic(c, a.rounds, a.nsub, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds, a.reeval_lib))


if __name__ == "__main__":
    main()
