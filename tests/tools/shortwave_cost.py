#!/usr/bin/env python3
"""GPU box: what shortwave COSZEN mode (include/elmk.h "shortwave") costs per step of elmk_run against REFERENCE mode.  Tier B, a grid
over the globe, 48 half-hour steps over 3-hourly records, graphs on, one context switching modes: per round each mode runs once
untimed (the first run after a change of mode captures its step again) and once timed, the order of the modes alternating from round
to round (an interleaved A/B).  Wall-clock ms per model step, median over the rounds; the REFERENCE medians are set beside the run
rows of profiles/r07_run_cost.jsonl ("b_run", the same step over hourly records).
python tests/tools/shortwave_cost.py [--cols 1000000,10000000] [--rounds 5] [--out profiles/r11_shortwave_cost.jsonl]
python tests/tools/shortwave_cost.py --only coszen --cols 1000000 --rounds 1     (one mode, for a kernel trace)"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from costlib import ROOT  # noqa: E402

DT, FORC_DT = CL.DT, 3 * 3600.0
NSTEPS = 48
SPR = int(FORC_DT // DT)
NREC = NSTEPS // SPR + 1
DAY0 = 171.0


def schedule():
    return CL.evolving_schedule(NSTEPS, DAY0, SPR, (5, 6))


def rec_times():
    return DAY0 + 1.0 + np.arange(NREC) * FORC_DT / 86400.0


def setup(cols):
    return CL.run_context(cols, "B", geography_seed=None, slots=NREC, max_steps=NSTEPS, records=NREC)


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

    def run():
        D.run(DT, steps)
        D.run_diagnostics()

    for r in range(rounds):
        for m in CL.interleave(r, modes):
            set_mode(D, m)
            D.run(DT, steps[:1])  # untimed: the capture of the mode's run step
            D.run_diagnostics()
            res[m].append(CL.wall_ms(D, run) / NSTEPS)
    D.close()
    med = CL.medians(res)
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
    a = CL.cli("1000000,10000000", 5, (CL.arg("--only", choices=["reference", "coszen"], default=None),), out=True)
    modes = [a.only] if a.only else ["reference", "coszen"]
    CL.emit_each(a, lambda c: measure(c, a.rounds, modes))


if __name__ == "__main__":
    main()
