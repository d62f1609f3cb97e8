#!/usr/bin/env python3
"""GPU box: what downscaling TOPO mode (include/elmk.h "downscaling") costs per step of elmk_run against OFF.  Tier B, a grid over the
globe, 48 half-hour steps over 3-hourly per-column records, graphs on, one context switching modes: OFF, TOPO, and TOPO with longwave
groups (regrid.owner_map, about 150 columns per group).  Column elevations lie within +-1500 m of the forcing's surface height.  Per
round each mode runs once untimed (the first run after a change captures its step again) and once timed, the order of the modes
reversing from round to round (an interleaved A/B).  Wall-clock ms per model step, median over the rounds.
python tests/tools/downscaling_cost.py [--cols 1000000,10000000] [--rounds 5] [--out profiles/r12_downscaling_cost.jsonl]
python tests/tools/downscaling_cost.py --only topo_groups --cols 1000000 --rounds 1     (one mode, for a kernel trace)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import regrid as RG  # noqa: E402

DT, FORC_DT = CL.DT, 3 * 3600.0
NSTEPS = 48
SPR = int(FORC_DT // DT)
NREC = NSTEPS // SPR + 1
DAY0 = 171.0
MODES = ["off", "topo", "topo_groups"]
GROUP_COLS = 150


def schedule():
    return CL.evolving_schedule(NSTEPS, DAY0, SPR, (5, 6))


def setup(cols):
    D = CL.base_context(cols, "B", geography=CL.synth.global_grid(cols))
    rng = np.random.default_rng(12)
    hf = 200.0 + 1500.0 * rng.random(cols)
    D.set_column_elevation(hf + rng.uniform(-1500.0, 1500.0, cols), hf)
    CL.resident_records(D, NREC, NSTEPS, records=NREC)
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

    def run():
        D.run(DT, steps)
        D.run_diagnostics()

    for r in range(rounds):
        for m in CL.interleave(r, modes):
            set_mode(D, m, groups)
            D.run(DT, steps[:1])  # untimed: the capture of the mode's run step
            D.run_diagnostics()
            res[m].append(CL.wall_ms(D, run) / NSTEPS)
    D.close()
    med = CL.medians(res)
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
    a = CL.cli("1000000,10000000", 5, (CL.arg("--only", choices=MODES, default=None),), out=True)
    modes = [a.only] if a.only else MODES
    CL.emit_each(a, lambda c: measure(c, a.rounds, modes))


if __name__ == "__main__":
    main()
