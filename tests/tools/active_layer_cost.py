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
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402
from elmkernels_amd import _lib as L  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = 1800.0
# soil layers thawed from the top (280 K over 260 K), bytes per column on the tally
TIERS = {"alt_thawed": (15, 32), "alt_frozen": (0, 136), "alt_front": (7, 104)}


def load_parent(path):
    """A build of the parent commit has every symbol but the new ones: declare what it exports."""
    lib = C.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            assert name.startswith("elmk_active_layer_"), name
            continue
        fn.restype, fn.argtypes = res, args
    L._libs[path] = lib


def build(cols, lib_path=None, feature=True):
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
    if feature:
        D.active_layer_enable()
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
    ms = back_to_back(D, D.active_layer_update)
    D.upload("t_soisno", soil, layout=st.LAYOUT_SOA)
    return ms


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


def measure(cols, rounds, run_steps):
    D = build(cols)
    steps = schedule(run_steps)
    soil = D.download("t_soisno", layout=st.LAYOUT_SOA)
    accum.add_t10(D, DT)
    res = {m: [] for m in tuple(TIERS) + ("accum_t10", "run", "run+alt")}
    for r in range(rounds):
        for tier in (tuple(TIERS) if r % 2 == 0 else tuple(TIERS)[::-1]):
            res[tier].append(tier_ms(D, tier, soil))
        res["accum_t10"].append(back_to_back(D, D.accum_update))
        order = (("run", 0), ("run+alt", st.RUN_ALT)) if r % 2 == 0 else (("run+alt", st.RUN_ALT), ("run", 0))
        for key, flags in order:
            res[key].append(run_ms(D, steps, flags))
    med = {k: float(np.median(v)) for k, v in res.items()}
    D.close()
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
           "spread": {k: spread(v) for k, v in res.items()}, "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9,
           "run_step_with_over_without": med["run+alt"] / med["run"], "run_step_added_ms": med["run+alt"] - med["run"]}
    for tier, (_, nbytes) in TIERS.items():
        out[tier + "_bytes"] = nbytes * cols
        out[tier + "_GBps"] = nbytes * cols / (med[tier] * 1e-3) / 1e9
        out[tier + "_over_accum_t10"] = med[tier] / med["accum_t10"]
    return out


def ab(cols, rounds, run_steps, lib_b):
    A, B = build(cols), build(cols, lib_path=lib_b)
    steps = schedule(run_steps)
    soil = A.download("t_soisno", layout=st.LAYOUT_SOA)
    pair = (("product", A), ("variant", B))
    res = {k: {m: [] for m in tuple(TIERS) + ("run+alt",)} for k, _ in pair}
    for r in range(rounds):
        turn = pair if r % 2 == 0 else pair[::-1]
        for tier in TIERS:
            for key, D in turn:
                res[key][tier].append(tier_ms(D, tier, soil))
        for key, D in turn:
            res[key]["run+alt"].append(run_ms(D, steps, st.RUN_ALT))
    out = {"columns": cols, "rounds": rounds, "run_steps": run_steps, "variant": os.path.basename(lib_b), "ms_all": res,
           "ms_median": {k: {m: float(np.median(v)) for m, v in d.items()} for k, d in res.items()},
           "spread": {k: {m: spread(v) for m, v in d.items()} for k, d in res.items()}}
    A.close()
    B.close()
    return out


def parent(cols, rounds, run_steps, lib_parent, parent_first):
    """The parent's library has no elmk_active_layer_*: neither context enables the feature, both run the unflagged step.  The second
    context of a process has run a step faster than the first at 1 M columns whatever the library, so both orders are recorded."""
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
            "first_context": "parent" if parent_first else "this", "run_ms_all": res,
            "run_ms_median": med, "spread": {k: spread(v) for k, v in res.items()}, "this_over_parent": med["this"] / med["parent"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=6)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-first", action="store_true")
    a = ap.parse_args()
    for c in [int(x) for x in a.cols.split(",")]:
        if a.ab:
            r = ab(c, a.rounds, a.run_steps, a.ab)
        elif a.parent:
            r = parent(c, a.rounds, a.run_steps, a.parent, a.parent_first)
        else:
            r = measure(c, a.rounds, a.run_steps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
