#!/usr/bin/env python3
"""GPU box: what the floodplain infiltration costs beside the three stages it extends, alone and inside elmk_run.  A tool of its own on
cost_routing.py's network and contexts, cost_routing_kinematic.py's parameters and cost_routing_inundation.py's banks; those tools and
their records stay what they are.  (Not called *_cost.py: tests/test_cost_tools_host.py pins the number of those.)

default mode (--cols N1,N2 are column counts, one cell per column): interleaved over `rounds` repeats, in one process, 40 calls back to
  back each:
    hyd_plain                 elmk_soil_hydrology, the extension off
    hyd_rof_none / _tenth / _all   the ROF form with no cell, every tenth cell, every cell flooded (a column of a flooded cell reads
                              cellof, WF, FLOOD_FRAC and area, 28 bytes, and every column writes the three rows, 24)
    k1_plain, k1_land         elmk_routing at nsub = 1 (the K1 launch and one sub-step) without and with the LAND form (8 bytes per term
                              and 24 per cell more)
  and the ratios over the plain forms.
--run: per column count, four columns per cell, nsub = 4: the run step with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE |
  ELMK_RUN_ROUTING under the inundation against the same with the extension on, a tenth of the cells over their banks, the snapshot
  restored before every run.
--parent LIB: the extension-off run step and hydrology launch alternated between this build and LIB, a build of the parent commit's
  library, two contexts of one process taking turns.  --parent-first: the parent's context is created first.  --parent2 LIB2: a second
  copy of the parent in this build's place, the spread two copies of one source show - the spread that decides whether "off" costs
  nothing.
Prints one JSON line per count (profiles/r26_floodplain_infiltration_cost.jsonl).
python tests/tools/cost_floodplain_infiltration.py [--cols 200000,4000000] [--rounds 5] [--run] [--run-steps 6]
                                                   [--parent LIB [--parent-first] [--parent2 LIB2]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cost_routing as CR  # noqa: E402
import cost_routing_inundation as CI  # noqa: E402
import cost_routing_kinematic as CK  # noqa: E402
import costlib as CL  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = CR.CALLS
TIERS = ("none", "tenth", "all")
BANKS = {"none": "dry", "tenth": "tenth", "all": "all"}  # cost_routing_inundation's tiers
ROF_BYTES = {"read_flooded": 4 + 3 * 8, "written": 3 * 8}


def rivers_on(D, cells, tier, nsub):
    """The kinematic scheme with the inundation of a tier on D's routing, and one call, so that FLOOD_FRAC holds the tier's floods."""
    CK.kw_on(D, cells)
    CI.flood_on(D, cells, BANKS[tier])
    D.routing(DT)


def measure(cols, rounds):
    D = CR.build(cols, nsub=1)
    D.water_balance_begin()
    D.water_balance(DT)
    res = {k: [] for k in ("hyd_plain",) + tuple(f"hyd_rof_{t}" for t in TIERS) + ("k1_plain", "k1_land")}
    flooded = {}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            tier = key.rsplit("_", 1)[1] if key.startswith("hyd_rof") else "tenth"
            rivers_on(D, cols, tier, 1)
            on = key.startswith("hyd_rof") or key == "k1_land"
            if on:
                D.floodplain_infiltration_enable()
            D.soil_hydrology_init()
            call = (lambda: D.soil_hydrology(DT)) if key.startswith("hyd") else (lambda: D.routing(DT))
            res[key].append(CL.back_to_back(D, call, CALLS))
            if key.startswith("hyd_rof"):
                flooded[key] = float((D.floodplain_infiltration_read(st.FPI_FRAC) > 0.0).mean())
            if on:
                D.floodplain_infiltration_clear()
            D.routing_inundation_clear()
            D.routing_kinematic_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols, "rounds": rounds, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "flooded_share": flooded, "rof_bytes_per_column": ROF_BYTES,
            "over_plain": {**{f"hyd_rof_{t}": med[f"hyd_rof_{t}"] / med["hyd_plain"] for t in TIERS}, "k1_land": med["k1_land"] / med["k1_plain"]}}


def measure_run(cols, rounds, run_steps):
    D = CR.build(cols, per_cell=4, nsub=4)
    steps = CL.schedule(run_steps)
    flags = CR.UNFLAGGED | st.RUN_ROUTING
    res = {"run+flood": [], "run+infiltration": []}
    CK.kw_on(D, cols // 4)
    CI.flood_on(D, cols // 4, "tenth")
    for r in range(rounds):
        for key in CL.interleave(r, res):
            D.soil_hydrology_init()
            if key == "run+infiltration":
                D.floodplain_infiltration_enable()
            res[key].append(CL.run_ms(D, steps, flags))
            if key == "run+infiltration":
                D.floodplain_infiltration_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "cells": cols // 4, "nsub": 4, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "run_step_infiltration_over_flood": med["run+infiltration"] / med["run+flood"],
            "run_step_infiltration_added_ms": med["run+infiltration"] - med["run+flood"]}


def parent_off(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent has the inundation and not the extension: both contexts turn the inundation on and take turns at the flagged run step
    and at the hydrology launch."""
    steps = CL.schedule(run_steps)
    flags = CR.UNFLAGGED | st.RUN_ROUTING

    def build(n, p):
        D = CR.build(n, lib_path=p, per_cell=4, nsub=4)
        CK.kw_on(D, n // 4)
        CI.flood_on(D, n // 4, "tenth")
        return D

    def run_step(D):
        D.soil_hydrology_init()
        return CL.run_ms(D, steps, flags)

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], build,
                             {"run_step": run_step, "hydrology": lambda D: CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS)},
                             first="parent" if parent_first else "this", optional=("elmk_floodplain_infiltration",))
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"],
            "this_over_parent": {k: c["median"]["this"][k] / c["median"]["parent"][k] for k in ("run_step", "hydrology")}}


def main():
    a = CL.cli("200000,4000000", 5, (CR.RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent_off(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
