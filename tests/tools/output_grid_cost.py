#!/usr/bin/env python3
"""GPU box: what output on a grid costs (include/elmk.h "output grid").  Tier A state, an ownership map (regrid.owner_map) of the
columns onto 67 420 cells - the land cells of a 0.5-degree grid - with the columns of a cell numbered contiguously ("contiguous") and
the same cells over permuted columns ("shuffled").  Per column count and map it reports, interleaved over `rounds` repeats:
  - elmk_download_gridded of one fp64 field level, against elmk_download of the level plus the host regrid.apply_aggregate (one
    thread) that a driver would otherwise run;
  - the bytes floor of one aggregated row: nnz x (4 + 8) of map terms + the source bytes touched + ncells x (8 + 8) (ptr, result),
    and the copy-probe rate (elmk_copy_bandwidth) to set it against;
  - the step time of physics alone, with a 12-flux AVG tape on the columns, and with the same tape on the cells (gridded entries),
    and the accumulate launches alone.
--kernel-loop MAP: only N gridded downloads of one map, for a rocprofv3 --kernel-trace --stats run of its own;
--stats DB: read that run's results database and append the aggregate kernel's time with the rate it implies at the floor bytes.
python tests/tools/output_grid_cost.py [--cols 1000000,10000000] [--rounds 3] [--out profiles/r09_output_grid_cost.jsonl]"""
import os
import sqlite3
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import regrid as RG  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
NCELLS = 67420
FILL = 1.0e36
FLUXES = ["eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "eflx_soil_grnd", "eflx_lwrad_out", "fsa", "fsr", "sabg", "sabv",
          "qflx_tran_veg", "t_ref2m", "q_ref2m"]


def owner(ncols, kind, seed=7):
    rng = np.random.default_rng(seed)
    cell = np.sort(rng.integers(0, NCELLS, ncols))
    if kind == "shuffled":
        cell = cell[rng.permutation(ncols)]
    return RG.owner_map(cell, rng.random(ncols) + 0.5, NCELLS)


def floor_bytes(ptr, ncols):
    return int(ptr[-1]) * 12 + ncols * 8 + NCELLS * 16  # every column is owned: each source element is touched once


def build(cols):
    return CL.base_context(cols)


def measure(cols, rounds, steps):
    D = build(cols)
    maps = {k: owner(cols, k) for k in ("contiguous", "shuffled")}
    out = np.empty(cols)
    res = {}
    for r in range(rounds):
        for kind, (ptr, col, w) in maps.items():
            D.history_clear()
            D.set_output_grid(ptr, col, w, FILL)
            R = res.setdefault(kind, {m: [] for m in ("dl_gridded", "dl_column", "dl_column+host", "phys", "phys+acc_col", "phys+acc_grid",
                                                       "acc_col", "acc_grid")})
            R["dl_gridded"].append(CL.back_to_back(D, lambda: D.download_gridded("t_grnd"), 20))
            R["dl_column"].append(CL.back_to_back(D, lambda: D.download("t_grnd", out=out), 5))
            R["dl_column+host"].append(CL.back_to_back(D, lambda: RG.apply_aggregate(ptr, col, w, D.download("t_grnd", out=out), FILL), 3))

            def phys():
                D.restore_fields()
                st.advance_physics(D, DT)

            def phys_acc():
                phys()
                D.history_accumulate()

            R["phys"].append(CL.back_to_back(D, phys, steps))
            for tag, add in (("col", D.history_add), ("grid", D.gridded_history_add)):
                D.history_clear()
                for k in FLUXES:
                    add(0, k, "avg")
                R[f"phys+acc_{tag}"].append(CL.back_to_back(D, phys_acc, steps))
                R[f"acc_{tag}"].append(CL.back_to_back(D, D.history_accumulate, 4 * steps))
    D.history_clear()
    bw0 = D.copy_bandwidth(1 << 30, 20, 0)
    bw_best = max([bw0] + [D.copy_bandwidth(1 << 30, 20, s) for s in (1, 2, 3)])
    lines = []
    for kind, (ptr, col, w) in maps.items():
        med = CL.medians(res[kind])
        fb = floor_bytes(ptr, cols)
        lines.append({
            "tool": "output_grid_cost", "columns": cols, "cells": NCELLS, "map": kind, "nnz": int(ptr[-1]), "rounds": rounds,
            "unit": "ms (wall clock, median over rounds)", "ms_median": med, "ms_all": res[kind],
            "floor_bytes_per_row": fb, "copy_bandwidth_GBps_shape0": bw0, "copy_bandwidth_GBps_best": bw_best,
            "floor_ms_at_copy_best": fb / (bw_best * 1e9) * 1e3,
            "dl_gridded_speedup_over_dl_column+host": med["dl_column+host"] / med["dl_gridded"],
            "step_added_ms_grid_tape": med["phys+acc_grid"] - med["phys"], "step_added_ms_column_tape": med["phys+acc_col"] - med["phys"],
        })
    D.close()
    return lines


def kernel_loop(cols, kind, n):
    D = build(cols)
    ptr, col, w = owner(cols, kind)
    D.set_output_grid(ptr, col, w, FILL)
    for _ in range(n):
        D.download_gridded("t_grnd")
    D.close()


def stats_line(path, cols, kind):
    """The aggregate kernel's dispatches in a rocprofv3 --kernel-trace results database (run_results.db, the `kernels` view)."""
    db = sqlite3.connect(path)
    ns = np.array([r[0] for r in db.execute("select duration from kernels where name like '%k_ogrid_aggregate%'")], dtype=np.float64)
    ptr, _, _ = owner(cols, kind)
    fb = floor_bytes(ptr, cols)
    med = float(np.median(ns))
    return {"tool": "output_grid_cost", "columns": cols, "cells": NCELLS, "map": kind, "kernel": "k_ogrid_aggregate",
            "source": "rocprofv3 --kernel-trace --stats", "calls": int(ns.size), "kernel_us_median": med / 1e3,
            "kernel_us_mean": float(ns.mean()) / 1e3, "floor_bytes_per_row": fb, "GBps_at_floor_bytes": fb / med}


def main():
    a = CL.cli("1000000,10000000", 3, (CL.arg("--steps", type=int, default=6), CL.arg("--kernel-loop", default=None, help="contiguous | shuffled"),
                                         CL.arg("--stats", default=None), CL.arg("--map", default="contiguous")), out=True)
    if a.kernel_loop:
        kernel_loop(a.cols[0], a.kernel_loop, 50)
    elif a.stats:
        CL.emit(stats_line(a.stats, a.cols[0], a.map), a.out)
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds, a.steps))


if __name__ == "__main__":
    main()
