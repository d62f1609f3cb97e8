#!/usr/bin/env python3
"""GPU box: what the water balance and history entries over feature rows cost, alone and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  balance       elmk_water_balance with all three pointers NULL (W1 - W8: k_water_balance, the two reduction stages over three rows,
                the census), 20 calls back to back; 616 B per column on the byte tally (fp64 state, with the frost rows 624)
  conservation  launch for launch the nearest existing thing, elmk_evaluate_conservation: it synchronises and downloads 192 bytes
                per call, so `balance+sync` (elmk_water_balance with pointers, which synchronises and downloads 88 bytes) stands beside
                it; 636 B per column on the same tally (snow-free columns; up to 100 B more under snow)
  begin         elmk_water_balance_begin (W0: 16 B read, 8 B written per column)
  t10           elmk_accum_update with the one T10 entry (the 10-day running mean of t_ref2m into t10), the existing launch nearest to W0
  run+hyd       elmk_run per step with ELMK_RUN_HYDROLOGY, the snapshot restored before every run
  run+hyd+wb    the same with ELMK_RUN_WATER_BALANCE
  run+hyd+wb+4  the same with ELMK_RUN_HISTORY and four AVG row entries on one tape (QRUNOFF, ENDWB, ZWT, QFLX_DRAIN)
Prints one JSON line per column count (profiles/r18_water_balance_cost.jsonl), with the spread (max - min) / median of every mode.
--ab LIB      the stage alone, alternated between this build and LIB, the same sources built with -DELMK_WB_NT=1
              (make -C elmkernels_amd/csrc variant V=wbnt VFLAGS=-DELMK_WB_NT=1): the nontemporal-store A/B
--parent LIB [--parent2 LIB2]  the unflagged run step alone, alternated between this build and LIB, a build of the parent commit's
              library; with --parent2, a second build of the parent takes turns as well, and the spread between the two parents is the
              margin this build's step has to lie in
python tests/tools/water_balance_cost.py [--cols 1000000,10000000] [--rounds 3] [--run-steps 6] [--ab LIB | --parent LIB [--parent2 LIB2]]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
import hydrology_cost as HC  # noqa: E402
from elmkernels_amd import hydrology as hy  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
BALANCE_BYTES = 616       # 67 x 8 read by k_water_balance, 6 x 8 written, 3 x 8 read by stage 1 of the reduction, 8 by the census
CONSERVATION_BYTES = 636  # 63 x 8 + 4 read by k_conservation on a snow-free column, 8 x 8 written, 8 x 8 read by stage 1
NEW = ("elmk_water_balance", "elmk_run_water_balance", "elmk_column_history_add_row", "elmk_gridded_history_add_row")
CALLS = HC.CALLS


def build(cols, lib_path=None, feature=True):
    D = HC.build(cols, lib_path=lib_path, feature=feature)
    if feature:
        D.water_balance_enable(1.0e-9)
    return D


def measure(cols, rounds, run_steps):
    D = build(cols)
    t10 = D.accum_add("t_ref2m", "runmean", 480, "t10")
    D.accum_init(t10)
    steps = CL.schedule(run_steps)
    D.water_balance_begin()
    alone = {"balance": lambda: D.water_balance(DT, read=False), "balance+sync": lambda: D.water_balance(DT),
             "conservation": lambda: st.kokkos_evaluate_conservation(D, DT), "begin": D.water_balance_begin, "t10": D.accum_update}
    runs = {"run+hyd": st.RUN_HYDROLOGY, "run+hyd+wb": st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE,
            "run+hyd+wb+4": st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_HISTORY}
    res = {m: [] for m in list(alone) + list(runs)}
    for r in range(rounds):
        for key in CL.interleave(r, alone):
            res[key].append(CL.back_to_back(D, alone[key], CALLS))
        for key in CL.interleave(r, runs):
            if key == "run+hyd+wb+4":
                for fam, which in (("water_balance", hy.WB_QRUNOFF), ("water_balance", hy.WB_ENDWB), ("hydrology", hy.ZWT), ("hydrology", hy.QFLX_DRAIN)):
                    D.history_add_row(0, fam, which, "avg")
            D.soil_hydrology_init()
            res[key].append(CL.run_ms(D, steps, runs[key]))
            D.history_clear()
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "balance_bytes": BALANCE_BYTES * cols, "conservation_bytes": CONSERVATION_BYTES * cols,
            "balance_TBps": BALANCE_BYTES * cols / (med["balance"] * 1e-3) / 1e12,
            "bytes_ratio": BALANCE_BYTES / CONSERVATION_BYTES, "time_ratio_synced": med["balance+sync"] / med["conservation"],
            "time_ratio_launches": med["balance"] / med["conservation"], "begin_over_t10": med["begin"] / med["t10"],
            "run_step_wb_added_ms": med["run+hyd+wb"] - med["run+hyd"], "run_step_wb_over_hyd": med["run+hyd+wb"] / med["run+hyd"],
            "run_step_4_entries_added_ms": med["run+hyd+wb+4"] - med["run+hyd+wb"]}


def store_ab(cols, rounds, lib_nt):
    """The stage alone on two contexts in one process, plain stores (this build) and nontemporal stores (lib_nt), taking turns."""
    def begin(ctx):
        for D in ctx.values():
            D.water_balance_begin()

    c = CL.compare_libraries(cols, rounds, [("plain", None), ("nontemporal", lib_nt)], lambda n, p: build(n, lib_path=p),
                             lambda D: CL.back_to_back(D, lambda: D.water_balance(DT, read=False), CALLS), baseline="plain", prepare=begin)
    return {"columns": cols, "rounds": rounds, "ab": os.path.basename(lib_nt), "ms_all": c["all"], "ms_median": c["median"],
            "spread": c["spread"], "nontemporal_over_plain": c["nontemporal_over_plain"]}


def parent(cols, rounds, run_steps, lib_parent, lib_parent2):
    """A build of the parent commit has none of the new entry points: no context enables a feature, all run the unflagged step."""
    libs = [("this", None), ("parent", lib_parent)] + ([("parent2", lib_parent2)] if lib_parent2 else [])
    steps = CL.schedule(run_steps)
    c = CL.compare_libraries(cols, rounds, libs, lambda n, p: HC.build(n, lib_path=p, feature=False), lambda D: CL.run_ms(D, steps, 0),
                             optional=NEW + ("elmk_soil_hydrology", "elmk_active_layer"), baseline="parent")
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "libraries": {k: os.path.basename(p) if p else "this build" for k, p in libs},
           "run_ms_all": c["all"], "run_ms_median": c["median"], "spread": c["spread"], "this_over_parent": c["this_over_parent"]}
    if lib_parent2:
        out["parent2_over_parent"] = c["parent2_over_parent"]
    return out


def main():
    a = CL.cli("1000000,10000000", 3, (CL.RUN_STEPS, CL.AB, CL.PARENT, CL.PARENT2))

    def one(c):
        if a.ab:
            return store_ab(c, a.rounds, a.ab)
        if a.parent:
            return parent(c, a.rounds, a.run_steps, a.parent, a.parent2)
        return measure(c, a.rounds, a.run_steps)

    CL.emit_each(a, one)


if __name__ == "__main__":
    main()
