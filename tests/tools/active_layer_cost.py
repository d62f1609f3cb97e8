#!/usr/bin/env python3
"""GPU box: what the active layer thickness costs, next to the accumulated-field update as the streaming yardstick and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  alt_thawed  elmk_active_layer_update with every soil level at 280 K: every lane leaves the search at the first (bottom) level;
              32 B per column on the tally (8 B t_soisno, 8 B zsoi, 8 B altmax read, 8 B alt written; the first update also
              writes altmax and altmax_indx)
  alt_frozen  the same with every level at 260 K: all fifteen levels are read; 136 B per column (120 B t_soisno, 8 B altmax, 8 B alt)
  alt_front   soil layers 0 .. 6 at 280 K over layers 7 .. 14 at 260 K, a thaw front at mid depth: the search reads layers 14 .. 6
              and leaves; 104 B per column (72 B t_soisno, 16 B zsoi, 8 B altmax, 8 B alt) against 152 B when all fifteen are read
  accum_t10   elmk_accum_update with the single t10 entry (k_accum.hip: 32 B per column, two launches): the yardstick
  run         elmk_run per step without ELMK_RUN_ALT, the snapshot restored before every run
  run+alt     the same with ELMK_RUN_ALT
Prints one JSON line per column count (profiles/r15_active_layer_cost.jsonl).
--ab LIB: alt_thawed, alt_frozen and run+alt alone, interleaved between the product library and LIB (a build of the same ABI), for
the A/Bs of the unit's two switches:
  make -C elmkernels_amd/csrc variant V=alt_noexit FLAGS_k_active_layer=-DELMK_ALT_EARLY_EXIT=0     (every lane loads all fifteen levels)
  make -C elmkernels_amd/csrc variant V=alt_nt3 FLAGS_k_active_layer=-DELMK_STATE_NT=3             (1 = loads, 2 = stores, 3 = both)
--parent LIB: the unflagged run step alone, alternated between this build and LIB, a build of the parent commit's library
(git worktree add ../parent HEAD~1 && make -C ../parent/elmkernels_amd/csrc): the unflagged step must not have moved.
python tests/tools/active_layer_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--ab LIB | --parent LIB [--parent-first]]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
# soil layers thawed from the top (280 K over 260 K), bytes per column on the tally
TIERS = {"alt_thawed": (15, 32), "alt_frozen": (0, 136), "alt_front": (7, 104)}
CALLS = 40  # launches of a back-to-back series


def build(cols, lib_path=None, feature=True):
    D = CL.run_context(cols, lib_path=lib_path)
    if feature:
        D.active_layer_enable()
    return D


_TIER_SOIL = {}


def tier_ms(D, tier, soil):
    """The update back to back on a uniform soil column; t_soisno is put back afterwards (the run modes restore their own snapshot)."""
    key = (tier, D.ncols)
    if key not in _TIER_SOIL:
        _TIER_SOIL.clear()  # (one tier's array at a time: 1.6 GB at 10 M columns)
        a = np.full((20, D.ncols), 260.0)
        a[5:5 + TIERS[tier][0]] = 280.0
        _TIER_SOIL[key] = a
    D.upload("t_soisno", _TIER_SOIL[key], layout=st.LAYOUT_SOA)
    ms = CL.back_to_back(D, D.active_layer_update, CALLS)
    D.upload("t_soisno", soil, layout=st.LAYOUT_SOA)
    return ms


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = CL.schedule(run_steps)
    soil = D.download("t_soisno", layout=st.LAYOUT_SOA)
    accum.add_t10(D, DT)
    res = {m: [] for m in tuple(TIERS) + ("accum_t10", "run", "run+alt")}
    for r in range(rounds):
        for tier in CL.interleave(r, TIERS):
            res[tier].append(tier_ms(D, tier, soil))
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
        for key, flags in CL.interleave(r, (("run", 0), ("run+alt", st.RUN_ALT))):
            res[key].append(CL.run_ms(D, steps, flags))
    med = CL.medians(res)
    D.close()
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
           "spread": CL.spreads(res), "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9,
           "run_step_with_over_without": med["run+alt"] / med["run"], "run_step_added_ms": med["run+alt"] - med["run"]}
    for tier, (_, nbytes) in TIERS.items():
        out[tier + "_bytes"] = nbytes * cols
        out[tier + "_GBps"] = nbytes * cols / (med[tier] * 1e-3) / 1e9
        out[tier + "_over_accum_t10"] = med[tier] / med["accum_t10"]
    return out


def ab(cols, rounds, run_steps, lib_b):
    steps = CL.schedule(run_steps)
    soil = []  # the product context's soil temperatures, put back after every tier
    modes = {tier: (lambda D, tier=tier: tier_ms(D, tier, soil[0])) for tier in TIERS}
    modes["run+alt"] = lambda D: CL.run_ms(D, steps, st.RUN_ALT)
    c = CL.compare_libraries(cols, rounds, [("product", None), ("variant", lib_b)], lambda n, p: build(n, lib_path=p), modes,
                             prepare=lambda ctx: soil.append(ctx["product"].download("t_soisno", layout=st.LAYOUT_SOA)))
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "variant": os.path.basename(lib_b), "ms_all": c["all"],
            "ms_median": c["median"], "spread": c["spread"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first):
    """The parent's library has no elmk_active_layer_*: neither context enables the feature, both run the unflagged step.  The second
    context of a process has run a step faster than the first at 1 M columns whatever the library, so both orders are recorded."""
    steps = CL.schedule(run_steps)
    c = CL.compare_libraries(cols, rounds, [("this", None), ("parent", lib_parent)], lambda n, p: build(n, lib_path=p, feature=False),
                             lambda D: CL.run_ms(D, steps, 0), first="parent" if parent_first else "this",
                             optional=("elmk_active_layer_",), baseline="parent")
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "first_context": "parent" if parent_first else "this", "run_ms_all": c["all"],
            "run_ms_median": c["median"], "spread": c["spread"], "this_over_parent": c["this_over_parent"]}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.AB, CL.PARENT, CL.PARENT_FIRST))

    def one(c):
        if a.ab:
            return ab(c, a.rounds, a.run_steps, a.ab)
        if a.parent:
            return parent(c, a.rounds, a.run_steps, a.parent, a.parent_first)
        return measure(c, a.rounds, a.run_steps)

    CL.emit_each(a, one)


if __name__ == "__main__":
    main()
