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
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402
from elmkernels_amd import _lib as L  # noqa: E402
from elmkernels_amd import hydrology as hy  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = 1800.0
BYTES_PER_COLUMN = 1196


def load_parent(path):
    """A build of the parent commit has every symbol but the new ones."""
    L.load(path, optional=("elmk_soil_hydrology",))


def build(cols, lib_path=None, feature=True):
    D, _ = bench.build_state(cols, 0, "A", 0x5EEDE1A0, lib_path=lib_path)
    D.set_snow_age_tables(synth.snow_age_tables())
    D.set_graph(True)
    lat, lon = synth.global_grid(cols, seed=11)
    D.set_column_geography(lat, lon)
    D.run_reserve(2, 64)
    for k in st.SERIES_FORCING + st.SERIES_PHENOLOGY:
        D.series_upload(k, 0, D.download(k, layout=st.LAYOUT_SOA))
    if feature:
        D.soil_hydrology_enable()
        one = hy.hksat_from_texture(np.full((1, hy.N), 45.0), np.full((1, hy.N), 20.0), np.full((1, hy.N), 10.0), np.geomspace(0.007, 2.9, hy.N)[None, :])
        D.soil_hydrology_set_params(np.ascontiguousarray(np.broadcast_to(one, (hy.N, cols))), 0.4, float(hy.h2osfc_thresh(np.array([0.02]))[0]),
                                    float(hy.k_wet(np.array([2.0]))[0]), float(hy.rsub_top_max(np.array([2.0]))[0]))
        D.soil_hydrology_init()
    return D


def schedule(n):
    S = np.zeros(n, st.RUN_STEP_DTYPE)
    for s in range(n):
        ddoy = 180.25 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), 0
        w2 = np.full(8, (s + 0.5) / n)
        S[s]["forc_wt1"], S[s]["forc_wt2"] = 1.0 - w2, w2
        S[s]["month1"], S[s]["month2"], S[s]["month_wt1"], S[s]["month_wt2"] = 0, 1, 0.6, 0.4
    return S


def back_to_back(D, fn, n=20):
    fn()
    D.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    D.sync()
    return (time.perf_counter() - t0) / n * 1e3


def run_ms(D, steps, flags, n=3):
    def once():
        D.restore_fields()
        D.run(DT, steps, flags)
    once()
    D.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        once()
    D.sync()
    return (time.perf_counter() - t0) / (n * len(steps)) * 1e3


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = schedule(run_steps)
    res = {m: [] for m in ("stage", "mixed", "run", "run+hyd")}
    zw = np.array([0.01, 0.05, 0.3, 1.0, 2.5, 3.7, 3.9, 8.8, 12.0])[np.arange(cols) % 9]
    wa = np.full(cols, 4000.0)
    for r in range(rounds):
        for key in (("stage", "mixed") if r % 2 == 0 else ("mixed", "stage")):
            if key == "mixed":
                D.soil_hydrology_init(zw, wa)
            else:
                D.soil_hydrology_init()
            res[key].append(back_to_back(D, lambda: D.soil_hydrology(DT)))
        D.soil_hydrology_init()
        order = (("run", 0), ("run+hyd", st.RUN_HYDROLOGY)) if r % 2 == 0 else (("run+hyd", st.RUN_HYDROLOGY), ("run", 0))
        for key, flags in order:
            res[key].append(run_ms(D, steps, flags))
            D.soil_hydrology_init()
    med = {k: float(np.median(v)) for k, v in res.items()}
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": {k: spread(v) for k, v in res.items()}, "stage_bytes": BYTES_PER_COLUMN * cols,
            "stage_TBps": BYTES_PER_COLUMN * cols / (med["stage"] * 1e-3) / 1e12,
            "mixed_TBps": BYTES_PER_COLUMN * cols / (med["mixed"] * 1e-3) / 1e12, "mixed_over_stage": med["mixed"] / med["stage"], "run_step_with_over_without": med["run+hyd"] / med["run"],
            "run_step_added_ms": med["run+hyd"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first):
    """The parent's library has no elmk_soil_hydrology*: neither context enables the feature, both run the unflagged step."""
    load_parent(lib_parent)
    if parent_first:
        B, A = build(cols, lib_path=lib_parent, feature=False), build(cols, feature=False)
    else:
        A, B = build(cols, feature=False), build(cols, lib_path=lib_parent, feature=False)
    steps = schedule(run_steps)
    pair = (("this", A), ("parent", B))
    res = {k: [] for k, _ in pair}
    for r in range(rounds):
        for key, D in (pair if r % 2 == 0 else pair[::-1]):
            res[key].append(run_ms(D, steps, 0))
    med = {k: float(np.median(v)) for k, v in res.items()}
    A.close()
    B.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "first_context": "parent" if parent_first else "this", "run_ms_all": res, "run_ms_median": med,
            "spread": {k: spread(v) for k, v in res.items()}, "this_over_parent": med["this"] / med["parent"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=6)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-first", action="store_true")
    a = ap.parse_args()
    for c in [int(x) for x in a.cols.split(",")]:
        r = parent(c, a.rounds, a.run_steps, a.parent, a.parent_first) if a.parent else measure(c, a.rounds, a.run_steps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
