#!/usr/bin/env python3
"""GPU box: what shortwave COSZEN mode (include/elmk.h "shortwave") costs per step of elmk_run against REFERENCE mode.  Tier B, a grid
over the globe, 48 half-hour steps over 3-hourly records, graphs on, one context switching modes: per round each mode runs once
untimed (the first run after a change of mode captures its step again) and once timed, the order of the modes alternating from round
to round (an interleaved A/B).  Wall-clock ms per model step, median over the rounds; the REFERENCE medians are set beside the run
rows of profiles/r07_run_cost.jsonl ("b_run", the same step over hourly records).
python tests/tools/shortwave_cost.py [--cols 1000000,10000000] [--rounds 5] [--out profiles/r11_shortwave_cost.jsonl]
python tests/tools/shortwave_cost.py --only coszen --cols 1000000 --rounds 1     (one mode, for a kernel trace)"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT, FORC_DT = 1800.0, 3 * 3600.0
NSTEPS = 48
SPR = int(FORC_DT // DT)
NREC = NSTEPS // SPR + 1
DAY0 = 171.0
FORC, PHEN = st.SERIES_FORCING, st.SERIES_PHENOLOGY


def schedule():
    S = np.zeros(NSTEPS, st.RUN_STEP_DTYPE)
    for s in range(NSTEPS):
        ddoy = DAY0 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), s // SPR
        w2 = np.clip(((s % SPR) / SPR) + 0.03 * np.arange(8), 0.0, 1.0)
        S[s]["forc_wt2"], S[s]["forc_wt1"] = w2, 1.0 - w2
        S[s]["month1"], S[s]["month2"], S[s]["month_wt1"], S[s]["month_wt2"] = 5, 6, 0.4, 0.6
    return S


def rec_times():
    return DAY0 + 1.0 + np.arange(NREC) * FORC_DT / 86400.0


def setup(cols):
    D, _ = bench.build_state(cols, 0, "B", 0x5EEDE1A0)
    D.set_snow_age_tables(synth.snow_age_tables())
    D.set_graph(True)
    lat, lon = synth.global_grid(cols)
    D.set_column_geography(lat, lon)
    D.run_reserve(NREC, NSTEPS)
    for k in FORC:
        a = D.download(k, layout=st.LAYOUT_SOA)
        for r in range(NREC):
            D.series_upload(k, r, a[r % 2])
    for k in PHEN:
        a = D.download(k, layout=st.LAYOUT_SOA)
        D.series_upload(k, 0, np.stack([a[m % 2] for m in range(12)]))
    return D


def set_mode(D, mode):
    D.set_shortwave_mode(mode, FORC_DT)
    if mode == "coszen":
        D.series_record_times(0, rec_times())


def r07_run_ms(cols):
    path = os.path.join(ROOT, "profiles", "r07_run_cost.jsonl")
    if not os.path.exists(path):
        return None
    for line in open(path):
        r = json.loads(line)
        if r.get("columns") == cols:
            return r["median"]["b_run"]
    return None


def measure(cols, rounds, modes):
    D = setup(cols)
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
            set_mode(D, m)
            D.run(DT, steps[:1])  # untimed: the capture of the mode's run step
            D.run_diagnostics()
            res[m].append(timed())
    D.close()
    med = {m: float(np.median(v)) for m, v in res.items()}
    out = {"columns": cols, "tier": "B", "steps": NSTEPS, "records": NREC, "forc_dt": FORC_DT, "rounds": rounds,
           "unit": "ms per step (wall clock)", "median": med, "all": res}
    if "coszen" in med and "reference" in med:
        out["coszen_over_reference"] = med["coszen"] / med["reference"]
        out["coszen_within_2pct"] = bool(out["coszen_over_reference"] <= 1.02)
    ref07 = r07_run_ms(cols)
    if ref07 is not None and "reference" in med:
        out["r07_b_run"] = ref07
        out["reference_over_r07"] = med["reference"] / ref07
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cols", default="1000000,10000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["reference", "coszen"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    modes = [a.only] if a.only else ["reference", "coszen"]
    for c in [int(x) for x in a.cols.split(",")]:
        line = json.dumps(measure(c, a.rounds, modes))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
