#!/usr/bin/env python3
"""GPU box: what forcing on a coarser grid costs against per-column forcing (include/elmk.h "forcing grid").  Tier B, half-hour
steps over hourly records, a day of 48 steps as two runs of 24 (the second window's 12 records uploaded while the first run executes),
columns spread over the globe (synth.global_grid).  Per column count it reports, interleaved over `rounds` repeats (the modes take
turns inside every round):
  - ms per step (wall clock) of the per-column run and of grid-mode runs, at ncells = ncols / 16 and ncols / 150 (regular grids with
    nlon = 2 nlat), nearest and bilinear maps, with the columns in spatial order (sorted by their nearest cell) and shuffled;
  - the 12-record window upload alone, per column and in cells;
  - elmk_device_bytes of each mode;
  - the host apply_map time for one record of the 7 streams (what a host-side remap would cost per record), on one thread and
    split over --threads threads.
--ab LIB: the grid runs of one column count again with a second build of the library (e.g. the map loads with the nontemporal hint,
make -C elmkernels_amd/csrc variant V=gridnt VFLAGS=-DELMK_GRID_MAP_NT=1), interleaved round by round with the product.
--only MODE/ORDER: one mode only (e.g. "column/spatial", "grid/16/bilinear/spatial"), for a rocprofv3 --kernel-trace --stats run of its
own.
python tests/tools/forcing_grid_cost.py [--cols 1000000,10000000] [--rounds 3] [--out profiles/r08_forcing_grid_cost.jsonl]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from costlib import FORC, PHEN  # noqa: E402
from elmkernels_amd import regrid as RG  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

DT = CL.DT
NSTEPS, NREC, WINDOW = 48, 25, 24


def schedule():
    """The day of run_cost.py: hourly records from mid-January, the month bracket moving at half time."""
    return CL.evolving_schedule(NSTEPS, 13.875, 2, [(11, 0)] * (NSTEPS // 2) + [(0, 1)] * (NSTEPS // 2))


def grid_shape(ncells):
    nlat = max(1, int(round(np.sqrt(ncells / 2.0))))
    return 2 * nlat, nlat


def geography(ncols, order):
    lat, lon = synth.global_grid(ncols)
    if order == "spatial":  # columns numbered along the rows of a fine grid, as a land model's gridcells usually are
        nlon, nlat = grid_shape(ncols // 16)
        key = RG.nearest_map(np.degrees(lat), np.degrees(lon), nlon, nlat)[0][0]
        o = np.lexsort((lon, key))
        lat, lon = lat[o], lon[o]
    return lat, lon


class Case:
    """One context with its geography; host records alternate between two rows (the bytes moved are those of distinct records)."""

    def __init__(self, ncols, order, lib_path=None):
        self.lat, self.lon = geography(ncols, order)
        self.D = CL.base_context(ncols, "B", lib_path, geography=(self.lat, self.lon))
        self.rows = {}
        for k in FORC + PHEN:
            a = self.D.download(k, layout=st.LAYOUT_SOA)
            self.rows[k] = np.ascontiguousarray(np.stack([a[0], a[1]]))
        self.maps = {}

    def map(self, div, kind):
        key = (div, kind)
        if key not in self.maps:
            nlon, nlat = grid_shape(self.D.ncols // div)
            f = RG.nearest_map if kind == "nearest" else RG.bilinear_map
            idx, w = f(np.degrees(self.lat), np.degrees(self.lon), nlon, nlat)
            self.maps[key] = (idx, w, nlon * nlat)
        return self.maps[key]

    def reserve(self, mode):
        """mode: "column" or (div, kind).  Map + reservation + the phenology months + the first window's records."""
        D = self.D
        if mode == "column":
            D.clear_forcing_grid()
            self.n = D.ncols
        else:
            idx, w, ncells = self.map(*mode)
            D.set_forcing_grid(idx, w, ncells)
            self.n = ncells
        D.run_reserve(NREC, WINDOW)
        for k in PHEN:
            D.series_upload(k, 0, np.stack([self.rows[k][m % 2] for m in range(12)]))
        self.upload(0, self.split)

    def upload(self, lo, hi):
        for k in FORC:
            for r in range(lo, hi):
                self.D.series_upload(k, r, self.rows[k][r % 2][None, :self.n])

    split = int(schedule()[WINDOW - 1]["forc_slot"]) + 2  # records the first window reads: 0 .. split - 1

    def two_runs(self, steps):
        D = self.D

        def runs():
            D.run(DT, steps[:WINDOW])
            self.upload(self.split, NREC)
            D.run(DT, steps[WINDOW:])
            D.run_diagnostics()

        return CL.wall_ms(D, runs) / NSTEPS

    def window_upload(self):
        return CL.wall_ms(self.D, lambda: self.upload(self.split, self.split + 12))


def mode_name(m):
    return "column" if m == "column" else f"grid/{m[0]}/{m[1]}"


def host_apply_ms(case, div, kind, threads):
    """One record of the 7 streams remapped on the host: one thread, and columns split over `threads` threads."""
    idx, w, ncells = case.map(div, kind)
    rec = [case.rows[k][0][:ncells] for k in FORC]
    t0 = time.perf_counter()
    for a in rec:
        RG.apply_map(idx, w, a)
    one = (time.perf_counter() - t0) * 1e3
    bounds = np.linspace(0, idx.shape[1], threads + 1).astype(np.int64)
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        for a in rec:
            list(ex.map(lambda i: RG.apply_map(idx[:, bounds[i]:bounds[i + 1]], w[:, bounds[i]:bounds[i + 1]], a), range(threads)))
        many = (time.perf_counter() - t0) * 1e3
    return one, many


def measure(ncols, rounds, threads, only=None, ab=None):
    steps = schedule()
    modes = ["column"] + [(div, kind) for div in (16, 150) for kind in ("nearest", "bilinear")]
    orders = ("spatial", "shuffled")
    if only:  # "<mode>/<order>"
        mode, order = only.rsplit("/", 1)
        modes, orders = [m for m in modes if mode_name(m) == mode], (order,)
    out = []
    for order in orders:
        C = Case(ncols, order)
        B = Case(ncols, order, ab) if ab else None
        res = {mode_name(m): [] for m in modes}
        if B:
            res.update({mode_name(m) + "/ab": [] for m in modes if m != "column"})
        upl, dev = {}, {}
        for r in range(rounds + 1):  # round 0: warm-up (graph captures, first touches)
            for m in modes:
                C.reserve(m)
                ms = C.two_runs(steps)
                print(f"# {ncols} {order} round {r} {mode_name(m)}: {ms:.3f} ms per step", file=sys.stderr, flush=True)
                if r > 0:
                    res[mode_name(m)].append(ms)
                dev[mode_name(m)] = C.D.device_bytes
                if r == rounds:
                    upl[mode_name(m)] = C.window_upload()
                if B and m != "column":
                    B.reserve(m)
                    ms = B.two_runs(steps)
                    if r > 0:
                        res[mode_name(m) + "/ab"].append(ms)
        med = CL.medians({k: v for k, v in res.items() if v})
        rec = {"columns": ncols, "order": order, "tier": "B", "steps": NSTEPS, "runs": 2, "records": NREC, "rounds": rounds,
               "unit": "ms per step (wall clock)", "median": med, "all": res, "window12_upload_ms": upl, "device_bytes": dev,
               "ncells": {f"grid/{d}": int(np.prod(grid_shape(ncols // d))) for d in (16, 150)},
               "grid_over_column": {k: v / med["column"] for k, v in med.items() if k != "column" and "column" in med}}
        if ab:
            rec["ab_lib"] = os.path.basename(ab)
        if not only and order == "spatial":
            rec["host_apply_map_one_record_ms"] = {f"grid/{d}/{k}": dict(zip(("one_thread", f"{threads}_threads"), host_apply_ms(C, d, k, threads)))
                                                   for d in (16,) for k in ("nearest", "bilinear")}
        C.D.close()
        if B:
            B.D.close()
        out.append(rec)
    return out


def main():
    a = CL.cli("1000000,10000000", 3, (CL.arg("--threads", type=int, default=16), CL.arg("--only", default=None), CL.AB), out=True)
    CL.emit_each(a, lambda c: measure(c, a.rounds, a.threads, a.only, a.ab))


if __name__ == "__main__":
    main()
