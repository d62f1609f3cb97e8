#!/usr/bin/env python3
"""GPU box: what interpolating the aerosol deposition streams on the device costs, next to a streaming yardstick measured in the same
process, next to the eleven uploads it replaces, and inside elmk_run.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round; one warm-up call before each
timed batch):
  aer_n1      elmk_aerosol_deposition, nearest-cell map (npts = 1) onto ncells = 13 824 cells (ELM's 1.9 x 2.5 degree grid, 144 x 96),
              back to back.  Bytes on the tally 88 written + npad x 12 of map read per column: 100 B
  aer_n4      the same with the bilinear map (npts = 4): 136 B per column
  accum_1     elmk_accum_update with the single t10 entry (k_accum.hip: 32 B per column, two launches): the yardstick for a
              streaming kernel on this box
  upload_11   what the kernel replaces: eleven elmk_upload calls of [ncols] doubles from host memory
  run         elmk_run per step without ELMK_RUN_AEROSOL, the snapshot restored before every run
  run+aer     the same with ELMK_RUN_AEROSOL (the npts = 1 map)
  run_parent  (--parent-lib LIB) elmk_run per step without the flag on a build of the parent commit's sources, in a context of its
              own, taking turns with `run`: whether the unflagged run slowed down is judged against this, with the parent's own
              run-to-run spread (max - min over the rounds) as the margin
Prints one JSON line per column count (profiles/r14_aerosol_cost.jsonl).
python tests/tools/aerosol_cost.py [--cols 1000000,10000000] [--rounds 5] [--run-steps 6] [--parent-lib path/to/libelmk_parent.so]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import _lib as L  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import aerosol  # noqa: E402
from elmkernels_amd import regrid  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = CL.DT
NLON, NLAT = 144, 96
NCELLS = NLON * NLAT
CALLS = 40  # launches of a back-to-back series (upload_11: 3)


def build(cols, lib_path=None):
    lat, lon = synth.global_grid(cols, seed=11)
    D = CL.base_context(cols, lib_path=lib_path, geography=(lat, lon))
    CL.resident_records(D)
    return D, np.degrees(lat), np.degrees(lon)


def reserve(D, series, idx, w):
    D.aerosol_reserve(NCELLS, idx, w)
    for s in aerosol.STREAMS:
        D.aerosol_upload(s, 0, series[s])


def measure(cols, rounds, run_steps, parent_lib):
    D, lat, lon = build(cols)
    Pn = None
    if parent_lib:
        try:
            Pn = build(cols, lib_path=parent_lib)[0]
        except L.ElmkError as e:  # (two contexts of this size do not fit: the line then says so instead of a parent figure)
            print(f"parent context at {cols} columns: {e}", file=sys.stderr)
    steps = CL.schedule(run_steps)
    series = aerosol.synthetic_climatology(NCELLS, seed=1)
    maps = {"aer_n1": regrid.nearest_map(lat, lon, NLON, NLAT), "aer_n4": regrid.bilinear_map(lat, lon, NLON, NLAT)}
    host = [np.ascontiguousarray(D[f]) for f in aerosol.FIELDS]

    def upload_11():
        for f, a in zip(aerosol.FIELDS, host):
            D.upload(f, a)

    modes = ["aer_n1", "aer_n4", "accum_1", "upload_11", "run", "run+aer"] + (["run_parent"] if Pn else [])
    res = {m: [] for m in modes}
    for r in range(rounds):
        accum.add_t10(D, DT)
        res["accum_1"].append(CL.back_to_back(D, D.accum_update, CALLS))
        D.accum_clear()
        for key in CL.interleave(r, ("aer_n4", "aer_n1")):
            reserve(D, series, *maps[key])
            res[key].append(CL.back_to_back(D, lambda: D.aerosol_deposition(0, 1, 0.6, 0.4), CALLS))
        res["upload_11"].append(CL.back_to_back(D, upload_11, 3))
        reserve(D, series, *maps["aer_n1"])
        order = [("run", D, 0), ("run+aer", D, st.RUN_AEROSOL)] + ([("run_parent", Pn, 0)] if Pn else [])
        for key, ctx, flags in CL.interleave(r, order):
            res[key].append(CL.run_ms(ctx, steps, flags))
    med = CL.medians(res)
    spread = {k: float(max(v) - min(v)) for k, v in res.items()}  # in ms, not over the median: the parent's is the margin
    bw0 = D.copy_bandwidth(1 << 30, 20, 0)
    D.close()
    if Pn:
        Pn.close()
    gbps = lambda b, k: b * cols / (med[k] * 1e-3) / 1e9  # noqa: E731
    out = {
        "columns": cols, "ncells": NCELLS, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_spread": spread, "ms_all": res,
        "aer_n1_bytes_per_col": 100, "aer_n4_bytes_per_col": 136, "accum_1_bytes_per_col": 32,
        "aer_n1_GBps": gbps(100, "aer_n1"), "aer_n4_GBps": gbps(136, "aer_n4"), "accum_1_GBps": gbps(32, "accum_1"),
        "upload_11_over_aer_n1": med["upload_11"] / med["aer_n1"],
        "run_step_with_over_without": med["run+aer"] / med["run"], "run_step_added_ms": med["run+aer"] - med["run"],
        "copy_bandwidth_GBps_shape0": bw0,
    }
    out["aer_n1_rate_over_yardstick"] = out["aer_n1_GBps"] / out["accum_1_GBps"]
    out["aer_n4_rate_over_yardstick"] = out["aer_n4_GBps"] / out["accum_1_GBps"]
    if Pn:
        out["run_minus_parent_ms"] = med["run"] - med["run_parent"]
        out["parent_spread_ms"] = spread["run_parent"]
    return out


def main():
    a = CL.cli("1000000,10000000", 5, (CL.RUN_STEPS, CL.arg("--parent-lib", default=None)))
    if a.parent_lib:
        CL.load_build(a.parent_lib, optional=("elmk_aerosol_",))
    CL.emit_each(a, lambda c: measure(c, a.rounds, a.run_steps, a.parent_lib))


if __name__ == "__main__":
    main()
