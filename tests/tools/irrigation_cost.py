#!/usr/bin/env python3
"""GPU box: what the irrigation stage costs, next to the accumulated-field update as the streaming yardstick and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  irr_idle   elmk_irrigation with the columns in 48 longitude bands half an hour of local time apart, over the 900 s from a quarter past noon
             UTC, in which no band's clock passes 06:00, and no window open: no column applies or checks; 40 B per column on the tally (4 B sched, 8 B NLEFT, 4 B frac_veg_nosno, 8 B elai, 8 B btran read, 8 B QFLX_IRRIG written)
  irr_band   the same at a time of day at which one band's clock passes 06:00: the vegetated, stressed columns of that band - one column in 48 at most - walk the
             soil levels (and, from the second call on, apply as well); 40 B per column plus, per checking column, 4 B vtype, 8 B
             t_soisno and 8 B rootfr per level walked, 5 x 8 B per rooted level, 16 B RATE and NLEFT written and 8 + 4 + 16 B for the
             application (counted from the state as it stands)
  accum_t10  elmk_accum_update with the single t10 entry (k_accum.hip: 32 B per column, two launches): the yardstick
  run        elmk_run per step without ELMK_RUN_IRRIGATION, the snapshot restored before every run
  run+irr    the same with ELMK_RUN_IRRIGATION
Prints one JSON line per column count (profiles/r18_irrigation_cost.jsonl).
--parent LIB: the unflagged run step alone, alternated between this build and LIB, a build of the parent commit's library
(git worktree add ../parent HEAD~1 && make -C ../parent/elmkernels_amd/csrc): the unflagged step must not have moved.
--parent2 LIB2 with --parent: LIB2, a second build of the parent, takes this build's place: the difference of the two is the margin.
python tests/tools/irrigation_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--parent LIB [--parent-first] [--parent2 LIB2]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
IDLE_BYTES = 40
NOON = 43200
IDLE_DT = 900.0  # the idle tier's step: from a quarter past to the half hour, between the bands' clocks
CALLS = 40  # launches of a back-to-back series


def band_sched(cols):
    """48 longitude bands of equal size, band b half an hour of local time east of band b - 1."""
    return ((np.arange(cols, dtype=np.int64) * 48 // cols) * 1800).astype(np.int32)


def build(cols, lib_path=None, sched=None):
    D = CL.run_context(cols, lib_path=lib_path)
    if sched is not None:
        D.irrigation_enable(sched)
    return D


def checking_bytes(D, col0, n):
    """(columns that check, their bytes on the tally) of the band [col0, col0 + n) from the state as it stands: the levels a column
    walks end at its first frozen one, and a rooted level among them costs five more rows."""
    get = lambda k: D.download(k, col0=col0, n=n, layout=st.LAYOUT_SOA).astype(np.float64)  # noqa: E731
    checks = (get("frac_veg_nosno").reshape(-1) != 0) & (get("elai").reshape(-1) > 0.0) & (get("btran").reshape(-1) < 0.999999)
    t, root = get("t_soisno")[5:20][:, checks], get("rootfr")[:, checks]
    frozen = ~(t > 273.15) & ~np.isnan(t)
    walked = np.where(frozen.any(axis=0), frozen.argmax(axis=0), 15)
    lev = np.arange(15)[:, None]
    rooted = ((root > 0.0) & (lev < walked[None, :])).sum()
    nbytes = int(checks.sum()) * (4 + 16 + 8 + 4 + 16) + 8 * int(np.minimum(walked + 1, 15).sum()) + 8 * int(walked.sum()) + 40 * int(rooted)
    return int(checks.sum()), nbytes


def measure(cols, rounds, run_steps):
    sched = band_sched(cols)
    D = build(cols, sched=sched)
    steps = CL.schedule(run_steps)
    accum.add_t10(D, DT)
    # band 24 passes 06:00 local at tod = 21600 - 24 * 1800 (mod a day); in the 900 s from noon + 900 s no band does (every band is on a
    # half hour)
    tod_band = (21600 - 24 * 1800) % 86400
    band = np.nonzero(sched == 24 * 1800)[0]
    idle_tod = NOON + 900
    assert not (((idle_tod + sched.astype(np.int64)) % 86400 - 21600) % 86400 < IDLE_DT).any()
    assert (((tod_band + sched[band].astype(np.int64)) % 86400 - 21600) % 86400 < DT).all()
    res = {m: [] for m in ("irr_idle", "irr_band", "accum_t10", "run", "run+irr")}
    tally = []
    for r in range(rounds):
        for mode in CL.interleave(r, ("irr_idle", "irr_band")):
            D.irrigation_init()
            if mode == "irr_band":
                tally.append(checking_bytes(D, int(band[0]), band.size))
            launch = (lambda: D.irrigation(IDLE_DT, idle_tod)) if mode == "irr_idle" else (lambda: D.irrigation(DT, tod_band))
            res[mode].append(CL.back_to_back(D, launch, CALLS))
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
        D.irrigation_init()
        for key, flags in CL.interleave(r, (("run", 0), ("run+irr", st.RUN_IRRIGATION))):
            res[key].append(CL.run_ms(D, steps, flags))
    med = CL.medians(res)
    nchecks, check_bytes = tally[len(tally) // 2]
    band_bytes = IDLE_BYTES * cols + check_bytes
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": CL.spreads(res), "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9,
            "irr_idle_bytes": IDLE_BYTES * cols, "irr_idle_GBps": IDLE_BYTES * cols / (med["irr_idle"] * 1e-3) / 1e9,
            "irr_band_bytes": band_bytes, "irr_band_GBps": band_bytes / (med["irr_band"] * 1e-3) / 1e9, "band_columns": int(band.size),
            "checking_columns_per_round": [t[0] for t in tally],
            "irr_idle_over_accum_t10": med["irr_idle"] / med["accum_t10"], "irr_band_over_irr_idle": med["irr_band"] / med["irr_idle"],
            "run_step_with_over_without": med["run+irr"] / med["run"], "run_step_added_ms": med["run+irr"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent's library has no elmk_irrigation_*: neither context enables the feature, both run the unflagged step.  The second
    context of a process has run a step faster than the first at 1 M columns whatever the library, so both orders are recorded.
    lib_this: a second build of the parent in the place of this build - what two builds of the same sources differ by is the margin."""
    steps = CL.schedule(run_steps)
    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], lambda n, p: build(n, lib_path=p),
                             lambda D: CL.run_ms(D, steps, 0), first="parent" if parent_first else "this",
                             optional=("elmk_irrigation",), baseline="parent")
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this", "run_ms_all": c["all"],
            "run_ms_median": c["median"], "spread": c["spread"], "this_over_parent": c["this_over_parent"]}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2))
    CL.emit_each(a, lambda c: parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2) if a.parent else measure(c, a.rounds, a.run_steps))


if __name__ == "__main__":
    main()
