#!/usr/bin/env python3
"""GPU box: what downscaling TOPO mode (include/elmk.h "downscaling") costs per step of elmk_run against OFF.  Tier B, a grid over the
globe, 48 half-hour steps over 3-hourly per-column records, graphs on, one context switching modes: OFF, TOPO, and TOPO with longwave
groups (regrid.owner_map, about 150 columns per group).  Column elevations lie within +-1500 m of the forcing's surface height.  Per
round each mode runs once untimed (the first run after a change captures its step again) and once timed, the order of the modes
reversing from round to round (an interleaved A/B).  Wall-clock ms per model step, median over the rounds.
python tests/tools/downscaling_cost.py [--cols 1000000,10000000] [--rounds 5] [--out profiles/r12_downscaling_cost.jsonl]
python tests/tools/downscaling_cost.py --only topo_groups --cols 1000000 --rounds 1     (one mode, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from elmkernels_amd import regrid as RG  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT, FORC_DT = 1800.0, 3 * 3600.0
NSTEPS = 48
SPR = int(FORC_DT // DT)
NREC = NSTEPS // SPR + 1
DAY0 = 171.0
FORC, PHEN = st.SERIES_FORCING, st.SERIES_PHENOLOGY
MODES = ["off", "topo", "topo_groups"]
GROUP_COLS = 150


def schedule():
    S = np.zeros(NSTEPS, st.RUN_STEP_DTYPE)
    for s in range(NSTEPS):
        ddoy = DAY0 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), s // SPR
        w2 = np.clip(((s % SPR) / SPR) + 0.03 * np.arange(8), 0.0, 1.0)
        S[s]["forc_wt2"], S[s]["forc_wt1"] = w2, 1.0 - w2
        S[s]["month1"], S[s]["month2"], S[s]["month_wt1"], S[s]["month_wt2"] = 5, 6, 0.4, 0.6
    return S


def setup(cols):
    D, _ = bench.build_state(cols, 0, "B", 0x5EEDE1A0)
    D.set_snow_age_tables(synth.snow_age_tables())
    D.set_graph(True)
    lat, lon = synth.global_grid(cols)
    D.set_column_geography(lat, lon)
    rng = np.random.default_rng(12)
    hf = 200.0 + 1500.0 * rng.random(cols)
    D.set_column_elevation(hf + rng.uniform(-1500.0, 1500.0, cols), hf)
    D.run_reserve(NREC, NSTEPS)
    for k in FORC:
        a = D.download(k, layout=st.LAYOUT_SOA)
        for r in range(NREC):
            D.series_upload(k, r, a[r % 2])
    for k in PHEN:
        a = D.download(k, layout=st.LAYOUT_SOA)
        D.series_upload(k, 0, np.stack([a[m % 2] for m in range(12)]))
    ng = (cols + GROUP_COLS - 1) // GROUP_COLS
    groups = RG.owner_map(np.arange(cols) // GROUP_COLS, 0.5 + rng.random(cols), ng)
    return D, groups


def set_mode(D, mode, groups):
    if mode == "topo_groups":
        D.set_downscaling_groups(*groups)
    else:
        D.clear_downscaling_groups()
    D.set_downscaling("off" if mode == "off" else "topo")


def measure(cols, rounds, modes):
    D, groups = setup(cols)
    steps = schedule()
    res = {m: [] for m in modes}

    def timed():
        D.sync()
        t0 = time.perf_counter()
        D.run(DT, steps)
        D.run_diagnostics()
        return (time.perf_counter() - t0) * 1e3 / NSTEPS

    for r in range(rounds):
        order = modes if r % 2 == 0 else modes[::-1]
        for m in order:
            set_mode(D, m, groups)
            D.run(DT, steps[:1])  # untimed: the capture of the mode's run step
            D.run_diagnostics()
            res[m].append(timed())
    D.close()
    med = {m: float(np.median(v)) for m, v in res.items()}
    out = {"columns": cols, "tier": "B", "steps": NSTEPS, "records": NREC, "forc_dt": FORC_DT, "rounds": rounds,
           "groups": {"columns_per_group": GROUP_COLS, "ngroups": int(groups[0].size - 1)}, "unit": "ms per step (wall clock)",
           "median": med, "all": res}
    add_ratios(out)
    return out


def add_ratios(out):
    """mode / OFF of the medians, and the median over rounds of each round's own ratio: the box can change speed between rounds
    (two placement modes), which moves the medians of all modes but not a round's pairs"""
    med, res = out["median"], out["all"]
    for m in ("topo", "topo_groups"):
        if m in med and "off" in med:
            out[f"{m}_over_off"] = med[m] / med["off"]
            out[f"{m}_over_off_paired"] = float(np.median([a / b for a, b in zip(res[m], res["off"])]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=MODES, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = [a.only] if a.only else MODES
    for c in [int(x) for x in a.cols.split(",")]:
        line = json.dumps(measure(c, a.rounds, modes))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
