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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
EIGHT = ["t_ref2m", "q_ref2m", "t_grnd", "t_veg", "eflx_sh_tot", "eflx_lh_tot", "fsa", "h2osno"]
CALLS = 40  # launches of a back-to-back series


def build(cols, lib_path=None):
    return CL.run_context(cols, lib_path=lib_path)


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = CL.schedule(run_steps)

    res = {m: [] for m in ("hist_1", "accum_t10", "accum_8", "run", "run+accum")}
    for r in range(rounds):
        D.history_add(0, "t_ref2m", "avg")
        res["hist_1"].append(CL.back_to_back(D, D.history_accumulate, CALLS))
        D.history_clear()
        for k in EIGHT:
            D.accum_add(k, accum.RUNMEAN, 480)
        res["accum_8"].append(CL.back_to_back(D, D.accum_update, CALLS))
        D.accum_clear()
        accum.add_t10(D, DT)
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
        for key, flags in CL.interleave(r, (("run", 0), ("run+accum", st.RUN_ACCUM))):
            res[key].append(CL.run_ms(D, steps, flags))
        D.accum_clear()
    med = CL.medians(res)
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
    def t10(ctx):
        for D in ctx.values():
            accum.add_t10(D, DT)

    steps = CL.schedule(run_steps)
    modes = {"accum_t10": lambda D: CL.back_to_back(D, D.accum_update, CALLS), "run+accum": lambda D: CL.run_ms(D, steps, st.RUN_ACCUM)}
    c = CL.compare_libraries(cols, rounds, [("product", None), ("variant", lib_b)], build, modes, prepare=t10)
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "variant": os.path.basename(lib_b), "ms_all": c["all"],
            "ms_median": c["median"]}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.AB))
    CL.emit_each(a, lambda c: ab(c, a.rounds, a.run_steps, a.ab) if a.ab else measure(c, a.rounds, a.run_steps))


if __name__ == "__main__":
    main()
