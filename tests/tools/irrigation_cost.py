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
IDLE_BYTES = 40
NOON = 43200
IDLE_DT = 900.0  # the idle tier's step: from a quarter past to the half hour, between the bands' clocks


def load_parent(path):
    """A build of the parent commit has every symbol but the new ones: declare what it exports."""
    lib = C.CDLL(path)
    for name, (res, args) in L.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            assert name.startswith("elmk_irrigation"), name
            continue
        fn.restype, fn.argtypes = res, args
    L._libs[path] = lib


def band_sched(cols):
    """48 longitude bands of equal size, band b half an hour of local time east of band b - 1."""
    return ((np.arange(cols, dtype=np.int64) * 48 // cols) * 1800).astype(np.int32)


def build(cols, lib_path=None, sched=None):
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
    if sched is not None:
        D.irrigation_enable(sched)
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


def spread(v):
    return (max(v) - min(v)) / float(np.median(v))


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
    steps = schedule(run_steps)
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
        for mode in (("irr_idle", "irr_band") if r % 2 == 0 else ("irr_band", "irr_idle")):
            D.irrigation_init()
            if mode == "irr_band":
                tally.append(checking_bytes(D, int(band[0]), band.size))
            res[mode].append(back_to_back(D, (lambda: D.irrigation(IDLE_DT, idle_tod)) if mode == "irr_idle" else (lambda: D.irrigation(DT, tod_band))))
        res["accum_t10"].append(back_to_back(D, D.accum_update))
        D.irrigation_init()
        order = (("run", 0), ("run+irr", st.RUN_IRRIGATION)) if r % 2 == 0 else (("run+irr", st.RUN_IRRIGATION), ("run", 0))
        for key, flags in order:
            res[key].append(run_ms(D, steps, flags))
    med = {k: float(np.median(v)) for k, v in res.items()}
    nchecks, check_bytes = tally[len(tally) // 2]
    band_bytes = IDLE_BYTES * cols + check_bytes
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res,
            "spread": {k: spread(v) for k, v in res.items()}, "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9,
            "irr_idle_bytes": IDLE_BYTES * cols, "irr_idle_GBps": IDLE_BYTES * cols / (med["irr_idle"] * 1e-3) / 1e9,
            "irr_band_bytes": band_bytes, "irr_band_GBps": band_bytes / (med["irr_band"] * 1e-3) / 1e9, "band_columns": int(band.size),
            "checking_columns_per_round": [t[0] for t in tally],
            "irr_idle_over_accum_t10": med["irr_idle"] / med["accum_t10"], "irr_band_over_irr_idle": med["irr_band"] / med["irr_idle"],
            "run_step_with_over_without": med["run+irr"] / med["run"], "run_step_added_ms": med["run+irr"] - med["run"]}


def parent(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent's library has no elmk_irrigation_*: neither context enables the feature, both run the unflagged step.  The second
    context of a process has run a step faster than the first at 1 M columns whatever the library, so both orders are recorded.
    lib_this: a second build of the parent in the place of this build - what two builds of the same sources differ by is the margin."""
    load_parent(lib_parent)
    if lib_this:
        load_parent(lib_this)
    if parent_first:
        B, A = build(cols, lib_path=lib_parent), build(cols, lib_path=lib_this)
    else:
        A, B = build(cols, lib_path=lib_this), build(cols, lib_path=lib_parent)
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
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this", "run_ms_all": res,
            "run_ms_median": med, "spread": {k: spread(v) for k, v in res.items()}, "this_over_parent": med["this"] / med["parent"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--run-steps", type=int, default=6)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--parent2", default=None)
    a = ap.parse_args()
    for c in [int(x) for x in a.cols.split(",")]:
        r = parent(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2) if a.parent else measure(c, a.rounds, a.run_steps)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
