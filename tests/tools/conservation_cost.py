#!/usr/bin/env python3
"""GPU box: elmk_evaluate_conservation back to back on a benchmark state, for tests/tools/ab.sh to time its kernels (k_conservation,
k_cons_reduce1, k_cons_reduce2) under several builds of the library:
  AB_SCRIPT=tests/tools/conservation_cost.py AB_TIERS=A bash tests/tools/ab.sh <tag> "k_cons" <lib1.so> <lib2.so> ...
python tests/tools/conservation_cost.py [cols] [tiers] [calls]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import bench  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402
from elmkernels_amd import synth  # noqa: E402

cols = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
tiers = sys.argv[2] if len(sys.argv) > 2 else "A"
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
for tier in tiers:
    D, _ = bench.build_state(cols, 0, tier, 0x5EEDE1A0)
    D.set_snow_age_tables(synth.snow_age_tables())
    st.kokkos_init_timestep(D)
    st.advance_physics(D, 1800.0)  # the diagnostics of a real step
    for _ in range(5):
        mms = st.kokkos_evaluate_conservation(D, 1800.0)
    t0 = time.perf_counter()
    for _ in range(calls):
        mms = st.kokkos_evaluate_conservation(D, 1800.0)
    ms = (time.perf_counter() - t0) / calls * 1e3
    print(f"tier {tier} cols {cols}: elmk_evaluate_conservation {ms:.4f} ms per call, host clock, {calls} calls | errh2o sum {mms[1, 2]!r} netrad max {mms[7, 1]!r}",
          flush=True)
    D.close()
