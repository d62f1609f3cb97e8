#!/usr/bin/env python3
"""GPU box: what history accumulation costs next to the step it follows and the per-step download it replaces.

For each column count, interleaved over `rounds` repeats (the modes take turns inside every round):
  phys            elmk_advance_physics alone (the snapshot restored before every step, as bench.py does)
  phys+acc_a      the same plus elmk_history_accumulate of tape (a): 12 single-level fluxes, AVG
  phys+acc_b      the same plus elmk_history_accumulate of tape (b): the 19 PrimaryVars fields, AVG
  phys+dl_b       the same plus elmk_download of the 19 PrimaryVars fields every step (what a host-side average needs)
  acc_a, acc_b    elmk_history_accumulate alone, back to back: ms per launch and bytes moved per second
                  (bytes = per row and column: the stored source element + 16 B of fp64 accumulator read and write)
and elmk_copy_bandwidth (shape 0, and the best of shapes 0..3) from the same process.
--ab LIB: accumulate alone, interleaved between the product library and LIB (a build of the same ABI), for an A/B.
python tests/tools/history_cost.py [--cols 1000000,10000000] [--rounds 5] [--ab path/to/libelmk_variant.so]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import costlib as CL  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

DT = CL.DT
FLUXES = ["eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "eflx_soil_grnd", "eflx_lwrad_out", "fsa", "fsr", "sabg", "sabv",
          "qflx_tran_veg", "t_ref2m", "q_ref2m"]
PRIMARY = st.ELMInterface.PRIMARY_VARS


def tape_bytes(D, names):
    tot = 0
    for k in names:
        _, nlev, dt = D.fields[k]
        es = np.dtype(dt).itemsize
        if es == 8:
            es = D.lib.elmk_state_real_bytes()
        tot += nlev * D.ncols * (es + 16)
    return tot


def register(D, names):
    D.history_clear()
    for k in names:
        D.history_add(0, k, "avg")


def build(cols, lib_path=None):
    return CL.base_context(cols, lib_path=lib_path)


def measure(cols, rounds, steps):
    D = build(cols)
    out = {k: D.download(k) for k in PRIMARY}

    def phys():
        D.restore_fields()
        st.advance_physics(D, DT)

    def phys_acc():
        phys()
        D.history_accumulate()

    def phys_dl():
        phys()
        for k in PRIMARY:
            D.download(k, out=out[k])

    res = {m: [] for m in ("phys", "phys+acc_a", "phys+acc_b", "phys+dl_b", "acc_a", "acc_b")}
    for r in range(rounds):
        res["phys"].append(CL.back_to_back(D, phys, steps))
        register(D, FLUXES)
        res["phys+acc_a"].append(CL.back_to_back(D, phys_acc, steps))
        res["acc_a"].append(CL.back_to_back(D, D.history_accumulate, 4 * steps))
        register(D, PRIMARY)
        res["phys+acc_b"].append(CL.back_to_back(D, phys_acc, steps))
        res["acc_b"].append(CL.back_to_back(D, D.history_accumulate, 4 * steps))
        D.history_clear()
        res["phys+dl_b"].append(CL.back_to_back(D, phys_dl, max(2, steps // 3)))
    med = CL.medians(res)
    bytes_a, bytes_b = tape_bytes(D, FLUXES), tape_bytes(D, PRIMARY)
    bw0 = D.copy_bandwidth(1 << 30, 20, 0)
    bw_best = max([bw0] + [D.copy_bandwidth(1 << 30, 20, s) for s in (1, 2, 3)])
    D.close()
    return {
        "columns": cols, "rounds": rounds, "steps_per_round": steps,
        "ms_median": med, "ms_all": res,
        "acc_a_bytes": bytes_a, "acc_b_bytes": bytes_b,
        "acc_a_GBps": bytes_a / (med["acc_a"] * 1e-3) / 1e9, "acc_b_GBps": bytes_b / (med["acc_b"] * 1e-3) / 1e9,
        "copy_bandwidth_GBps_shape0": bw0, "copy_bandwidth_GBps_best": bw_best,
        "acc_b_fraction_of_copy_shape0": bytes_b / (med["acc_b"] * 1e-3) / 1e9 / bw0,
        "acc_b_fraction_of_copy_best": bytes_b / (med["acc_b"] * 1e-3) / 1e9 / bw_best,
        "step_cost_acc_b_over_dl_b": (med["phys+acc_b"] - med["phys"]) / max(med["phys+dl_b"] - med["phys"], 1e-9),
    }


def ab(cols, rounds, lib_b):
    def tape(names):
        def t(D):
            register(D, names)
            return CL.back_to_back(D, D.history_accumulate, 20)
        return t

    c = CL.compare_libraries(cols, rounds, [("product", None), ("variant", lib_b)], build, {"a": tape(FLUXES), "b": tape(PRIMARY)})
    return {"columns": cols, "rounds": rounds, "variant": os.path.basename(lib_b), "ms_all": c["all"], "ms_median": c["median"]}


def main():
    a = CL.cli("1000000,10000000", 5, (CL.arg("--steps", type=int, default=6), CL.AB))
    CL.emit_each(a, lambda c: ab(c, a.rounds, a.ab) if a.ab else measure(c, a.rounds, a.steps))


if __name__ == "__main__":
    main()
