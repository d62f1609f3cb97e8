#!/usr/bin/env python3
"""GPU box: what the frost-table extension of the soil hydrology stage costs (include/elmk.h "soil hydrology", F').

For each column count, interleaved over `rounds` repeats (off and on take turns inside every round, and change places from round to round):
  thawed      elmk_soil_hydrology back to back with every soil temperature above freezing: every lane of the extension takes branch B
              with nothing frozen (frost_B_thawed) and the stage goes on to F.1 and F.2
  permafrost  thaw fronts that cycle through layers 1 .. 9 in consecutive columns, the water table above the frost table in nine
              columns and below it in the next nine: every wave runs branches A and B under predicates
  Both: 20 launches on a state that evolves from launch to launch; the fields the stage writes, ZWT and WA are put back before every
  series, so off and on start from the same state.  `off` is the stage without the extension (k_soil_hydrology<false>), `on` with it.
  run         elmk_run per step with ELMK_RUN_HYDROLOGY on the permafrost tier, without and with the extension
`branches`: how many of the first 1152 columns take each branch of F' on the permafrost tier (hydrology.step on a download).
Prints one JSON line per column count (profiles/r17_frost_table_cost.jsonl), with the spread (max - min) / median of every mode.
--parent LIB: the stage without the extension alone, alternated between this build and LIB, a build of the parent commit's library, on
both tiers: `off` must not have moved, and the margin is this job's own spread.
python tests/tools/frost_table_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--parent LIB [--parent-first]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
import hydrology_cost as HC  # noqa: E402
from elmkernels_amd import hydrology as hy  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = HC.CALLS
# the stage's tally plus ten t_soisno, the parameter, three stored rows, and the loads F' repeats (dz and the ice:
# 20; hksat over the layers it sums: up to 10; three node depths)
BYTES_PER_COLUMN = {"off": HC.BYTES_PER_COLUMN, "on": HC.BYTES_PER_COLUMN + 8 * (10 + 1 + 3 + 20 + 10 + 3)}
WRITTEN = ("h2osoi_liq", "h2osoi_ice", "h2osoi_vol", "h2osfc")
S0, S1 = hy.NLEVSNO, hy.NLEVSNO + hy.N
NFRONT = 9


def tiers(D, cols):
    """t_soisno [cols, nlev] and ZWT of the two tiers, from the context's own soil grid."""
    t = D.download("t_soisno").astype(np.float64)
    z = D.download("zsoi").astype(np.float64)[:, S0:S1]
    c = np.arange(cols)
    thawed = t.copy()
    thawed[:, S0:S1] = 280.0
    front = 1 + c % NFRONT  # the first frozen layer
    perm = t.copy()
    perm[:, S0:S1] = np.where(np.arange(hy.N)[None, :] < front[:, None], 275.0, 270.0)
    ft = z[c, front]
    zwt = np.where((c // NFRONT) % 2 == 0, 0.5 * ft, ft + 1.0)
    return {"thawed": (thawed, None), "permafrost": (perm, zwt)}


def set_tier(D, tier, wa):
    t, zwt = tier
    D.upload("t_soisno", t)
    D.restore_fields()
    if zwt is None:
        D.soil_hydrology_init()
    else:
        D.soil_hydrology_init(zwt, wa)


def reset(D, tier, wa):
    D.restore_fields()
    if tier[1] is None:
        D.soil_hydrology_init()
    else:
        D.soil_hydrology_init(tier[1], wa)


def extension(D, on, q):
    D.soil_hydrology_frost_clear()
    if on:
        D.soil_hydrology_frost_enable(q)


def measure(cols, rounds, run_steps):
    D = HC.build(cols)
    D.snapshot_fields(WRITTEN)
    T = tiers(D, cols)
    wa = np.full(cols, 4000.0)
    q = hy.q_perch_max(np.full(cols, 2.0))
    res = {f"{t}_{m}": [] for t in T for m in ("off", "on")}
    res.update({"run_off": [], "run_on": []})
    for name, tier in T.items():
        set_tier(D, tier, wa)
        for r in range(rounds):
            for on in CL.interleave(r, (False, True)):
                extension(D, on, q)
                reset(D, tier, wa)
                res[f"{name}_{'on' if on else 'off'}"].append(CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS))
    # the branches of the permafrost tier, on the first columns (the tier is still set)
    extension(D, True, q)
    reset(D, T["permafrost"], wa)
    m = min(cols, 1152)
    rows = np.stack([D.soil_hydrology_read(w, 0, m) for w in range(hy.NROWS)])
    frost = np.stack([D.soil_hydrology_frost_read(w, 0, m) for w in range(hy.FROST_NROWS)])
    fields = {k: D.download(k, 0, m) for k in hy.READS + ("h2osoi_vol", "t_soisno")}
    marks = {}

    class Count:
        def add(self, k):
            marks[k] = marks.get(k, 0) + 1

    hy.step(fields, rows, DT, Count(), frost=frost)
    branches = {k: v for k, v in sorted(marks.items()) if k.startswith(("frost_", "perched_"))}
    # the run step: the snapshot of the benchmark again, so that its restore costs what it costs there
    D.restore_fields()
    D.snapshot_fields(CL.bench.RESTORE_FIELDS)
    steps = CL.schedule(run_steps)
    for r in range(rounds):
        for on in CL.interleave(r, (False, True)):
            extension(D, on, q)
            D.soil_hydrology_init(T["permafrost"][1], wa)
            D.upload("t_soisno", T["permafrost"][0])
            res["run_on" if on else "run_off"].append(CL.run_ms(D, steps, st.RUN_HYDROLOGY))
    med = CL.medians(res)
    D.close()
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
           "spread": CL.spreads(res), "bytes_per_column": BYTES_PER_COLUMN, "branches_first_columns": branches}
    for t in T:
        out[f"{t}_on_over_off"] = med[f"{t}_on"] / med[f"{t}_off"]
        out[f"{t}_TBps"] = {m: BYTES_PER_COLUMN[m] * cols / (med[f"{t}_{m}"] * 1e-3) / 1e12 for m in ("off", "on")}
    out["run_step_on_over_off"] = med["run_on"] / med["run_off"]
    out["run_step_added_ms"] = med["run_on"] - med["run_off"]
    return out


def parent(cols, rounds, lib_parent, parent_first):
    """The parent's library has the stage and none of elmk_soil_hydrology_frost_*: both contexts run the stage without the extension.
    One tier after the other, all rounds of a tier together: the contexts are opened once and take their turns inside each tier."""
    pair = CL.open_builds(cols, [("this", None), ("parent", lib_parent)], lambda n, p: HC.build(n, lib_path=p),
                          first="parent" if parent_first else "this", optional=("elmk_soil_hydrology_frost",))
    try:
        wa = np.full(cols, 4000.0)
        for D in pair.values():
            D.snapshot_fields(WRITTEN)
        T = tiers(pair["this"], cols)
        res = {f"{t}_{k}": [] for t in T for k in pair}
        for name, tier in T.items():
            for D in pair.values():
                set_tier(D, tier, wa)
            for r in range(rounds):
                for key in CL.interleave(r, pair):
                    D = pair[key]
                    reset(D, tier, wa)
                    res[f"{name}_{key}"].append(CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS))
    finally:
        CL.close_all(pair)
    med = CL.medians(res)
    return {"columns": cols, "rounds": rounds, "parent": os.path.basename(lib_parent), "first_context": "parent" if parent_first else "this",
            "stage_off_ms_all": res, "stage_off_ms_median": med, "spread": CL.spreads(res),
            "this_over_parent": {t: med[f"{t}_this"] / med[f"{t}_parent"] for t in T}}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST))
    CL.emit_each(a, lambda c: parent(c, a.rounds, a.parent, a.parent_first) if a.parent else measure(c, a.rounds, a.run_steps))


if __name__ == "__main__":
    main()
