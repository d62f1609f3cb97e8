#!/usr/bin/env python3
"""GPU box: what the hillslope lateral flow costs beside the soil hydrology stage it extends, alone and inside elmk_run.  A tool of its
own on hydrology_cost.py's context; that tool and its records stay what they are.  (Not called *_cost.py: tests/test_cost_tools_host.py
pins the number of those.)

default mode, per column count, interleaved over `rounds` repeats in one process, 20 calls back to back each, on water tables that
cycle through 0.3 .. 3.7 m in consecutive columns (every column has a transmissivity), ZWT and WA set again before every series:
    hyd_plain       elmk_soil_hydrology, the extension off (k_soil_hydrology<false, false>)
    hyd_lat_off     the extension on with every column on no hillslope: the two new launches store zeros and the LAT form runs F.1
    hyd_lat_chain5  chains of five columns, the fifth at the stream (map width 1)
    hyd_lat_star8   one column at the stream under eight uphill neighbours (map width 8)
    accum_t10       elmk_accum_update with the single t10 entry (k_accum.hip: 32 B per column): the streaming yardstick
  elmk_soil_hydrology enqueues the two new launches and the LAT form together and the ABI has no entry point for one of them alone, so
  what is timed is the three launches; `added_ms` is their time less hyd_plain's, and `added_TBps` is the added bytes over it.
  Bytes per column (fp64 state): L1 reads ZWT, 10 HKSAT, 11 zisoi, 10 dz, 10 ice, 10 watsat and elev (53 x 8) and down (4) and writes
  2 x 8; L2 reads down (4), the map (4 per slot), its own HEAD, TRANS, dist, width, area (40), the downhill HEAD and TRANS (16), per
  uphill neighbour HEAD, TRANS, dist, width (32) and writes 4 x 8; the LAT form reads down and QLAT_NET (12) more than the plain form.
--run: the run step with ELMK_RUN_HYDROLOGY without and with the extension (chains of five), the snapshot restored before every run.
--parent LIB: the extension off - the flagged run step and the hydrology launch alternated between this build and LIB, a build of the
  parent commit's library, two contexts of one process taking turns.  --parent-first: the parent's context is created first.
  --parent2 LIB2: a second copy of the parent in this build's place, the spread two copies of one source show - the spread that decides
  whether "off" costs nothing.
Prints one JSON line per count (profiles/r28_hillslope_cost.jsonl).
python tests/tools/cost_hillslope.py [--cols 1000000,10000000] [--rounds 5] [--run] [--run-steps 6]
                                     [--parent LIB [--parent-first] [--parent2 LIB2]] [--out FILE]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
import hydrology_cost as HC  # noqa: E402
from elmkernels_amd import accum  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
CALLS = HC.CALLS
SHAPES = ("off", "chain5", "star8")
MAP_WIDTH = {"off": 1, "chain5": 1, "star8": 8}
UPHILL = {"off": 0.0, "chain5": 4.0 / 5.0, "star8": 8.0 / 9.0}  # uphill neighbours per column, which is also the share with a downhill column
K_ANISO = 50.0
RUN = CL.arg("--run", action="store_true")


def added_bytes(shape):
    """What the extension moves per column beside the plain stage (the module's docstring)."""
    l1 = 53 * 8 + 4 + 2 * 8
    l2 = 4 + 4 * MAP_WIDTH[shape] + 40 + 4 * 8 + (0.0 if shape == "off" else 16.0 * UPHILL[shape] + 32.0 * UPHILL[shape])
    if shape == "off":  # (a column on no hillslope reads down in each launch and stores the six zeros)
        l1, l2 = 4 + 2 * 8, 4 + 4 * 8
    return {"head": l1, "flow": l2, "lat_form": 12, "sum": l1 + l2 + 12}


def geometry(cols, shape):
    """(down, dist, width, area, elev, k_aniso): every column on no hillslope; chains of five down 3 m per column; stars of nine, the
    eight uphill columns 3 m above the one at the stream.  A last group cut short by `cols` is a shorter hillslope of the same kind."""
    c = np.arange(cols)
    if shape == "off":
        down, elev = np.full(cols, -2), np.zeros(cols)
    elif shape == "chain5":
        down, elev = np.where(c % 5 == 0, -1, c - 1), 3.0 + 3.0 * (c % 5)
    else:
        down, elev = np.where(c % 9 == 0, -1, c - c % 9), np.where(c % 9 == 0, 3.0, 6.0)
    return down.astype(np.int32), 50.0, 30.0, 1500.0, elev, K_ANISO


def tables(cols):
    return np.array([0.3, 1.0, 2.5, 3.7])[np.arange(cols) % 4], np.full(cols, 4000.0)


def extension(D, shape, cols):
    D.hillslope_clear()
    if shape is not None:
        D.hillslope_enable(*geometry(cols, shape))


def measure(cols, rounds):
    D = HC.build(cols)
    accum.add_t10(D, DT)
    zw, wa = tables(cols)
    modes = {"hyd_plain": None, **{f"hyd_lat_{s}": s for s in SHAPES}}
    res = {k: [] for k in tuple(modes) + ("accum_t10",)}
    stream = {}
    for r in range(rounds):
        for key in CL.interleave(r, modes):
            extension(D, modes[key], cols)
            D.soil_hydrology_init(zw, wa)
            res[key].append(CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS))
            if modes[key] is not None:
                stream[key] = float(D.hillslope_budget()[0])
        res["accum_t10"].append(CL.back_to_back(D, D.accum_update, CALLS))
    med = CL.medians(res)
    D.close()
    out = {"columns": cols, "rounds": rounds, "ms_median": med, "ms_all": res, "spread": CL.spreads(res), "stream_discharge_m3s": stream,
           "plain_bytes_per_column": HC.BYTES_PER_COLUMN, "plain_TBps": HC.BYTES_PER_COLUMN * cols / (med["hyd_plain"] * 1e-3) / 1e12,
           "accum_t10_GBps": 32 * cols / (med["accum_t10"] * 1e-3) / 1e9, "added_bytes_per_column": {s: added_bytes(s) for s in SHAPES},
           "added_ms": {}, "added_TBps": {}, "over_plain": {}, "added_over_accum_t10": {}}
    for s in SHAPES:
        d = med[f"hyd_lat_{s}"] - med["hyd_plain"]
        out["added_ms"][s], out["over_plain"][s] = d, med[f"hyd_lat_{s}"] / med["hyd_plain"]
        out["added_TBps"][s] = added_bytes(s)["sum"] * cols / (d * 1e-3) / 1e12 if d > 0.0 else None
        out["added_over_accum_t10"][s] = d / med["accum_t10"]
    return out


def measure_run(cols, rounds, run_steps):
    D = HC.build(cols)
    D.snapshot_fields(CL.bench.RESTORE_FIELDS)
    steps = CL.schedule(run_steps)
    zw, wa = tables(cols)
    res = {"run+hyd": [], "run+hyd+lat": []}
    for r in range(rounds):
        for key in CL.interleave(r, res):
            extension(D, "chain5" if key == "run+hyd+lat" else None, cols)
            D.soil_hydrology_init(zw, wa)
            res[key].append(CL.run_ms(D, steps, st.RUN_HYDROLOGY))
    med = CL.medians(res)
    D.close()
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "ms_median": med, "ms_all": res, "spread": CL.spreads(res),
            "run_step_lat_over_hyd": med["run+hyd+lat"] / med["run+hyd"], "run_step_lat_added_ms": med["run+hyd+lat"] - med["run+hyd"]}


def parent_off(cols, rounds, run_steps, lib_parent, parent_first, lib_this=None):
    """The parent has the stage and not the extension: both contexts take turns at the flagged run step and at the hydrology launch."""
    steps = CL.schedule(run_steps)
    zw, wa = tables(cols)

    def build(n, p):
        D = HC.build(n, lib_path=p)
        D.snapshot_fields(CL.bench.RESTORE_FIELDS)
        return D

    def run_step(D):
        D.soil_hydrology_init(zw, wa)
        return CL.run_ms(D, steps, st.RUN_HYDROLOGY)

    def launch(D):
        D.soil_hydrology_init(zw, wa)
        return CL.back_to_back(D, lambda: D.soil_hydrology(DT), CALLS)

    c = CL.compare_libraries(cols, rounds, [("this", lib_this), ("parent", lib_parent)], build, {"run_step": run_step, "hydrology": launch},
                             first="parent" if parent_first else "this", optional=("elmk_hillslope",))
    return {"columns": cols, "rounds": rounds, "run_steps": run_steps, "parent": os.path.basename(lib_parent),
            "this": os.path.basename(lib_this) if lib_this else "libelmk.so", "first_context": "parent" if parent_first else "this",
            "ms_all": c["all"], "ms_median": c["median"], "spread": c["spread"],
            "this_over_parent": {k: c["median"]["this"][k] / c["median"]["parent"][k] for k in ("run_step", "hydrology")}}


def main():
    a = CL.cli("1000000,10000000", 5, (RUN, CL.RUN_STEPS, CL.PARENT, CL.PARENT_FIRST, CL.PARENT2), out=True)
    if a.parent:
        CL.emit_each(a, lambda c: parent_off(c, a.rounds, a.run_steps, a.parent, a.parent_first, a.parent2))
    elif a.run:
        CL.emit_each(a, lambda c: measure_run(c, a.rounds, a.run_steps))
    else:
        CL.emit_each(a, lambda c: measure(c, a.rounds))


if __name__ == "__main__":
    main()
