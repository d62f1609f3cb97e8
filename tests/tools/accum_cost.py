#!/usr/bin/env python3
"""GPU box: what updating the accumulated fields costs, next to the history accumulate it is modelled on and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  hist_1      elmk_history_accumulate with one single-level AVG entry (t_ref2m), back to back: the yardstick, 24 B per column
              (8 B source + 16 B accumulator read and write)
  accum_t10   elmk_accum_update with the single t10 entry (RUNMEAN of t_ref2m into t10): 32 B per column (8 B source, 16 B value
              read and write, 8 B destination); two launches, the second a one-thread kernel that advances the step count
  accum_8     elmk_accum_update with eight single-level entries (RUNMEAN, no destination: 24 B per column and entry)
  run         elmk_run per step without ELMK_RUN_ACCUM, the snapshot restored before every run
  run+accum   the same with ELMK_RUN_ACCUM and the t10 entry
Prints one JSON line per column count (profiles/r13_accum_cost.jsonl).
--ab LIB: accum_t10 and run+accum alone, interleaved between the product library and LIB (a build of the same ABI), for an A/B
(profiles/r13_accum_dst_nt_ab.jsonl: LIB a build whose destination store carried the nontemporal hint; the plain store won).
python tests/tools/accum_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--ab path/to/libelmk_variant.so]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = 1800.0
EIGHT = ["t_ref2m", "q_ref2m", "t_grnd", "t_veg", "eflx_sh_tot", "eflx_lh_tot", "fsa", "h2osno"]


def build(cols, lib_path=None):
    D, _ = bench.build_state(cols, 0, "A", 0x5EEDE1A0, lib_path=lib_path)
    D.set_snow_age_tables(synth.snow_age_tables())
    D.set_graph(True)
    lat, lon = synth.global_grid(cols, seed=11)
    D.set_column_geography(lat, lon)
    # a run over the two forcing records and two months the state already holds
    D.run_reserve(2, 64)
    for k in st.SERIES_FORCING + st.SERIES_PHENOLOGY:
        a = D.download(k, layout=st.LAYOUT_SOA)
        D.series_upload(k, 0, a)
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


def back_to_back(D, fn, n=40):
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


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = schedule(run_steps)

    res = {m: [] for m in ("hist_1", "accum_t10", "accum_8", "run", "run+accum")}
    for r in range(rounds):
        D.history_add(0, "t_ref2m", "avg")
        res["hist_1"].append(back_to_back(D, D.history_accumulate))
        D.history_clear()
        for k in EIGHT:
            D.accum_add(k, accum.RUNMEAN, 480)
        res["accum_8"].append(back_to_back(D, D.accum_update))
        D.accum_clear()
        accum.add_t10(D, DT)
        res["accum_t10"].append(back_to_back(D, D.accum_update))
        order = (("run", 0), ("run+accum", st.RUN_ACCUM)) if r % 2 == 0 else (("run+accum", st.RUN_ACCUM), ("run", 0))
        for key, flags in order:
            res[key].append(run_ms(D, steps, flags))
        D.accum_clear()
    med = {k: float(np.median(v)) for k, v in res.items()}
    bw0 = D.copy_bandwidth(1 << 30, 20, 0)
    D.close()
    return {
        "columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
        "hist_1_bytes": 24 * cols, "accum_t10_bytes": 32 * cols, "accum_8_bytes": 8 * 24 * cols,
        "hist_1_GBps": 24 * cols / (med["hist_1"] * 1e-3) / 1e9, "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9,
        "accum_8_GBps": 8 * 24 * cols / (med["accum_8"] * 1e-3) / 1e9,
        "accum_t10_over_hist_1": med["accum_t10"] / med["hist_1"], "expected_from_bytes": 32.0 / 24.0,
        "run_step_with_over_without": med["run+accum"] / med["run"], "run_step_added_ms": med["run+accum"] - med["run"],
        "copy_bandwidth_GBps_shape0": bw0,
    }


def ab(cols, rounds, run_steps, lib_b):
    A, B = build(cols), build(cols, lib_path=lib_b)
    steps = schedule(run_steps)
    for D in (A, B):
        accum.add_t10(D, DT)
    res = {k: {"accum_t10": [], "run+accum": []} for k in ("product", "variant")}
    for r in range(rounds):
        for key, D in ((("product", A), ("variant", B)) if r % 2 == 0 else (("variant", B), ("product", A))):
            res[key]["accum_t10"].append(back_to_back(D, D.accum_update))
        for key, D in ((("product", A), ("variant", B)) if r % 2 == 0 else (("variant", B), ("product", A))):
            res[key]["run+accum"].append(run_ms(D, steps, st.RUN_ACCUM))
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "variant": os.path.basename(lib_b), "ms_all": res,
           "ms_median": {k: {m: float(np.median(v)) for m, v in d.items()} for k, d in res.items()}}
    A.close()
    B.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=6)
    ap.add_argument("--ab", default=None)
    a = ap.parse_args()
    for c in [int(x) for x in a.cols.split(",")]:
        r = ab(c, a.rounds, a.run_steps, a.ab) if a.ab else measure(c, a.rounds, a.run_steps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
