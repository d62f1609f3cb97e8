#!/usr/bin/env python3
"""GPU box: what the soil hydrology stage costs, alone and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  stage      elmk_soil_hydrology back to back on the cold-start water table of the benchmark's state: the table is below the column
             (jwt == N) in every lane, so no lane takes a walk of the water table and nothing diverges - the cheapest case;
             1196 B per column on the byte tally of DESIGN.md section 20 (fp64 state)
  mixed      the same with the water table of consecutive columns cycling through 0.01 .. 12 m (jwt = 0, mid and N inside every
             wave): every wave executes the recharge branch and the walks of E and F under predicates beside the aquifer rows
  Both are 20 launches on a state that evolves from launch to launch; ZWT and WA are set again before every series.
  run        elmk_run per step without ELMK_RUN_HYDROLOGY, the snapshot restored before every run
  run+hyd    the same with ELMK_RUN_HYDROLOGY
Prints one JSON line per column count (profiles/r16_hydrology_cost.jsonl), with the spread (max - min) / median of every mode.
--parent LIB: the unflagged run step alone, alternated between this build and LIB, a build of the parent commit's library: the
unflagged step must not have moved.
python tests/tools/hydrology_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--parent LIB [--parent-first]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import hydrology as hy  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
BYTES_PER_COLUMN = 1196
CALLS = 20  # launches of a back-to-back series


def build(cols, lib_path=None, feature=True):
    D = CL.run_context(cols, lib_path=lib_path)
    if feature:
        D.soil_hydrology_enable()
        one = hy.hksat_from_texture(np.full((1, hy.N), 45.0), np.full((1, hy.N), 20.0), np.full((1, hy.N), 10.0), np.geomspace(0.007, 2.9, hy.N)[None, :])
        D.soil_hydrology_set_params(np.ascontiguousarray(np.broadcast_to(one, (hy.N, cols))), 0.4, float(hy.h2osfc_thresh(np.array([0.02]))[0]),
                                    float(hy.k_wet(np.array([2.0]))[0]), float(hy.rsub_top_max(np.array([2.0]))[0]))
        D.soil_hydrology_init()
    return D


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = CL.schedule(run_steps)
    res = {m: [] for m in ("stage", "mixed", "run", "run+hyd")}
    zw = np.array([0.01, 0.05, 0.3, 1.0, 2.5, 3.7, 3.9, 8.8, 12.0])[np.arange(cols) % 9]
    wa = np.full(cols, 4000.0)
    for r in range(rounds):
        for key in CL.interleave(r, ("stage", "mixed")):
            if key == "mixed":
                D.soil_hydrology_init(zw, wa)
            else:
                D.soil_hydrology_init()
            res[key].append(CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS))
        D.soil_hydrology_init()
        for key, flags in CL.interleave(r, (("run", 0), ("run+hyd", st.RUN_HYDROLOGY))):
            res[key].append(CL.run_ms(D, steps, flags))
            D.soil_hydrology_init()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "stage_bytes": BYTES_PER_COLUMN * cols,
            "stage_TBps": BYTES_PER_COLUMN * cols / (med["stage"] * 1e-3) / 1e12,
            "mixed_TBps": BYTES_PER_COLUMN * cols / (med["mixed"] * 1e-3) / 1e12, "mixed_over_stage": med["mixed"] / med["stage"], "run_step_with_over_without": med["run+hyd"] / med["run"],
            "run_step_added_ms": med["run+hyd"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first):
    """The parent's library has no elmk_soil_hydrology*: neither context enables the feature, both run the unflagged step."""
    steps = CL.schedule(run_steps)
    c = CL.compare_libraries(cols, rounds, [("this", None), ("parent", lib_parent)], lambda n, p: build(n, lib_path=p, feature=False),
                             lambda D: CL.run_ms(D, steps, 0), first="parent" if parent_first else "this",
                             optional=("elmk_soil_hydrology",), baseline="parent")
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "first_context": "parent" if parent_first else "this", "run_ms_all": c["all"], "run_ms_median": c["median"],
            "spread": c["spread"], "this_over_parent": c["this_over_parent"]}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST))
    CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first) if a.parent else measure(c, a.rounds, a.run_steps))


if __name__ == "__main__":
    main()
