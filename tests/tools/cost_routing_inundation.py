#!/usr/bin/env python3
"""GPU box: what the floodplain inundation costs beside the kinematic-wave scheme it extends, alone and inside elmk_run.  A tool of its
own on cost_routing.py's network and contexts and cost_routing_kinematic.py's parameters; those tools and their records stay what they
are.  (Not called *_cost.py: tests/test_cost_tools_host.py pins the number of those.)

default mode (--cols N1,N2 are cell counts): per count, one cell per column, cost_routing's network.  Interleaved over `rounds` repeats,
  in one process, 40 calls back to back each, nsub = 1 (two launches) and 8 (nine launches):
    kw_nsub*          elmk_routing with the kinematic-wave scheme, the extension off
    dry_nsub*         the flood form with no cell over its banks (banks of 1e4 m, floodplains empty)
    tenth_nsub*       every tenth cell over its banks (banks of 1 cm there, of 1e4 m elsewhere)
    all_nsub*         every cell over its banks (banks of 1 cm)
  and the ratios over kw.  Byte tally per cell of a middle sub-step (neither first nor last) on top of the kinematic sub-step's 176 (160
  streamed + 4 npad + the gathers): a cell inside its banks reads VC and WF, 16; a cell that exchanges reads ACHN, AF, E_0 .. E_10 and
  VB_1 .. VB_10 as well and writes WF, 16 + 184 + 8 = 208; the LAST sub-step writes the two diagnostics, 16 more.
--run: per column count, four columns per cell, nsub = 4: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE |
  ELMK_RUN_ROUTING under the kinematic scheme against the same with the extension on, a tenth of the cells over their banks, the
  snapshot restored before every run.
--parent LIB: the kinematic call with the extension off (--nsub sub-steps, one cell per column) alternated between this build and LIB, a
  build of the parent commit's library, two contexts of one process taking turns.  --parent-first: the parent's context is created
  first.  --parent2 LIB2: a second copy of the parent in this build's place, the spread two copies of one source show.
Prints one JSON line per count (profiles/r22_routing_inundation_cost.jsonl).
python tests/tools/cost_routing_inundation.py [--cols 200000,4000000] [--rounds 5] [--run] [--run-steps 6]
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
TIERS = ("dry", "tenth", "all")
KW_SUB_STEP_BYTES = 176


def banks(ncells, tier):
    """rdepth [ncells] of a tier and the profile [11, ncells]: steps of 0.2 m."""
    over = {"dry": np.zeros(ncells, bool), "tenth": np.arange(ncells) % 10 == 0, "all": np.ones(ncells, bool)}[tier]
    return np.where(over, 0.01, 1.0e4), np.repeat((0.2 * np.arange(rt.NPROF))[:, None], ncells, axis=1)


def flood_on(D, ncells, tier):
    rdepth, eprof = banks(ncells, tier)
    D.routing_inundation_enable(rdepth, eprof)
    D.routing_inundation_init(np.where(rdepth < 1.0, 2.0e6, 0.0))


def measure(cells, rounds):
    D = CR.build(cells)
    down = CR.network(cells)
    npad = rt.npad_of(rt.upstream_map(down))
    rng = np.random.default_rng(3)
    ddist, volr = np.exp(rng.uniform(np.log(2000.0), np.log(60000.0), cells)), rng.uniform(0.0, 1.0e6, cells)
    D.water_balance_begin()
    D.water_balance(DT)
    res = {f"{t}_nsub{n}": [] for n in (1, 8) for t in ("kw",) + TIERS}
    wet = {}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            tier, nsub = key.split("_nsub")
            D.routing_enable(down, ddist, np.full(cells, 1.0e8), rt.EFFVEL, int(nsub))
            D.routing_init(volr)
            CK.kw_on(D, cells)
            if tier != "kw":
                flood_on(D, cells, tier)
            res[key].append(CL.back_to_back(D, lambda: D.routing(DT), CALLS))
            if tier != "kw":
                wet[key] = float((D.routing_read(rt.WF) > 0.0).mean())  # the share of cells with a wet floodplain after the series
            D.routing_clear()
    med = CL.medians(res)
    D.close()
    sub = {t: (med[f"{t}_nsub8"] - med[f"{t}_nsub1"]) / 7 for t in ("kw",) + TIERS}
    share = {"dry": 0.0, "tenth": 0.1, "all": 1.0}
    added = {t: 16 + share[t] * (184 + 8) for t in TIERS}
    return {"cells": cells, "rounds": rounds, "npad": npad, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "launches": {"nsub1": 2, "nsub8": 9}, "wet_share_after": wet, "sub_step_ms": sub,
            "bytes_per_cell_sub_step": {"kw": KW_SUB_STEP_BYTES, **{t: KW_SUB_STEP_BYTES + added[t] for t in TIERS}},
            "over_kw": {f"{t}_nsub{n}": med[f"{t}_nsub{n}"] / med[f"kw_nsub{n}"] for n in (1, 8) for t in TIERS}}


def measure_run(cols, rounds, run_steps):
    D = CR.build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    flags = CR.UNFLAGGED | st.RUN_ROUTING
    res = {"run+kinematic": [], "run+flood": []}
    CK.kw_on(D, cols // 4)
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.soil_hydrology_init()
            if key == "run+flood":
                flood_on(D, cols // 4, "tenth")
            res[key].append(CL.run_ms(D, steps, flags))
            if key == "run+flood":
                D.routing_inundation_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_flood_over_kinematic": med["run+flood"] / med["run+kinematic"],
            "run_step_flood_added_ms": med["run+flood"] - med["run+kinematic"]}


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
                             first="parent" if parent_first else "this", optional=("elmk_routing_inundation",))
    return {"cells": cols, "nsub": nsub, "rounds": rounds, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"],
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
