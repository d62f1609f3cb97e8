#!/usr/bin/env python3
"""GPU box: what a 48-step evolving run costs per step, driven three ways (tier B, half-hour steps, hourly forcing records, a grid
that spans latitudes and longitudes; interleaved over `rounds` repeats, the loops taking turns inside every round):
  (a) stepwise   the loop of ELMInterface::advance (with solar geometry): per step elmk_solar_geometry, elmk_phenology,
                 elmk_get_forcing, elmk_init_timestep, elmk_advance_physics, elmk_evaluate_conservation, elmk_error_summary, and
                 both atm_* levels uploaded whenever the record bracket moves (mlai .. mhbot when the month bracket moves)
  (b) run        elmk_run of the 48 steps with all 25 records resident, then elmk_run_diagnostics
  (c) two runs   24 + 24 steps: the first window's records resident (uploaded during the previous pair of runs, as in a long
                 simulation), the second window's 12 records uploaded while the first run executes, the second run enqueued
                 before the first is read back, then elmk_run_diagnostics
Wall-clock ms per model step, median over the rounds.  Records alternate between two host rows (the host holds 3 x ncols per
stream instead of 25 x ncols); the physics does not care, the bytes moved are the same.
python tests/tools/run_cost.py [--cols 4096,65536,1000000,10000000] [--rounds 3] [--out profiles/r07_run_cost.jsonl]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from costlib import FORC, PHEN  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
NSTEPS, NREC, WINDOW = 48, 25, 24


def schedule():
    """Hourly records from mid-January, the month bracket moving at half time."""
    return CL.evolving_schedule(NSTEPS, 13.875, 2, [(11, 0)] * (NSTEPS // 2) + [(0, 1)] * (NSTEPS // 2))


def setup(cols):
    D = CL.base_context(cols, "B", geography=CL.synth.global_grid(cols))
    # host rows r0, r1, r0 per stream: the record pair (t, t + 1) is rows [t % 2, t % 2 + 2), one contiguous [2][ncols] block
    rows = {}
    for k in FORC + PHEN:
        a = D.download(k, layout=st.LAYOUT_SOA)
        rows[k] = np.ascontiguousarray(np.stack([a[0], a[1], a[0]]))
    return D, rows


def loop_stepwise(D, rows, steps):
    slot, month = None, None
    for p in steps:
        D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
        if slot != int(p["forc_slot"]):
            slot = int(p["forc_slot"])
            for k in FORC:
                D.upload(k, rows[k][slot % 2:slot % 2 + 2], layout=st.LAYOUT_SOA)
        if month != int(p["month1"]):
            month = int(p["month1"])
            for k in PHEN:
                D.upload(k, rows[k][month % 2:month % 2 + 2], layout=st.LAYOUT_SOA)
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"], False)
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        st.kokkos_evaluate_conservation(D, DT)
        D.error_summary()


def upload_slots(D, rows, lo, hi):
    for k in FORC:
        for r in range(lo, hi):
            D.series_upload(k, r, rows[k][r % 2])


def measure(cols, rounds):
    D, rows = setup(cols)
    steps = schedule()
    split = int(steps[WINDOW - 1]["forc_slot"]) + 2  # records the first window reads: 0 .. split - 1
    res = {"a_stepwise": [], "b_run": [], "c_two_runs": [], "c_window2_upload_alone": []}

    def t(fn):
        return CL.wall_ms(D, fn, sync_after=True)

    def b():
        D.run(DT, steps)
        D.run_diagnostics()

    def c():
        D.run(DT, steps[:WINDOW])
        upload_slots(D, rows, split, NREC)
        D.run(DT, steps[WINDOW:])
        D.run_diagnostics()

    for r in range(rounds + 1):  # round 0: warm-up (graph captures, first touches)
        ms_a = t(lambda: loop_stepwise(D, rows, steps))
        D.run_reserve(NREC, NSTEPS)
        upload_slots(D, rows, 0, NREC)
        for k in PHEN:
            D.series_upload(k, 0, np.stack([rows[k][m % 2] for m in range(12)]))
        ms_b = t(b)
        D.run_reserve(NREC, WINDOW)
        upload_slots(D, rows, 0, split)
        for k in PHEN:
            D.series_upload(k, 0, np.stack([rows[k][m % 2] for m in range(12)]))
        ms_c = t(c)
        ms_u = t(lambda: upload_slots(D, rows, split, NREC))
        if r > 0:
            res["a_stepwise"].append(ms_a / NSTEPS)
            res["b_run"].append(ms_b / NSTEPS)
            res["c_two_runs"].append(ms_c / NSTEPS)
            res["c_window2_upload_alone"].append(ms_u)
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "tier": "B", "steps": NSTEPS, "records": NREC, "rounds": rounds, "unit": "ms per step (wall clock)",
            "median": med, "all": res, "b_over_a": med["b_run"] / med["a_stepwise"], "c_over_b": med["c_two_runs"] / med["b_run"]}


def main():
    a = CL.cli("4096,65536,1000000,10000000", 3, out=True)
    CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
