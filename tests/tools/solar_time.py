#!/usr/bin/env python3
"""Device cost of per-column solar geometry, for a kernel-trace run of its own:

  rocprofv3 --kernel-trace --stats -d <dir> -o solar --output-format csv -- python3 tests/tools/solar_time.py <ncols> [tier] [steps]

One context of ncols columns (bench.py's synthetic state, a global lat / lon grid): `steps` launches of
k_solar_geometry, then `steps` fused steps (elmk_timestep7_fused) in scalar mode and `steps` in per-column mode on the same
coszen, the state restored from a snapshot before each step.  The kernel names tell the two modes apart (k_cf_iterate against
k_cf_dayl + k_cf_iterate_col_dayl); the HIP-event time of each fused step is printed here as well, per mode."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from elmkernels_amd import synth  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    tier = sys.argv[2] if len(sys.argv) > 2 else "B"
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    import bench

    D, _ = bench.build_state(n, 0, tier, 2024)  # the benchmark's state, its snapshot of the fields a step changes
    lat, lon = synth.global_grid(n, seed=7)
    D.set_column_geography(lat, lon)
    decday = 172.5
    for _ in range(steps):
        D.solar_geometry(synth.DTIME, decday, int(decday) - 1)
    D.sync()
    dayl, max_dayl = D.day_length()
    # the scalar run uses the northern group's day length, so both modes run the same canopy iteration on the northern half
    north = max_dayl > 0
    D.set_scalars(dayl=float(dayl[north][0]), max_dayl=float(max_dayl[north][0]))
    D.clear_column_geography()  # scalar mode, coszen as the solar step left it
    t_scalar = D.profile_steps(synth.DTIME, steps, fused=True)
    D.set_column_geography(lat, lon)
    D.solar_geometry(synth.DTIME, decday, int(decday) - 1)  # (the same coszen again)
    t_col = D.profile_steps(synth.DTIME, steps, fused=True)
    print(f"ncols {n} tier {tier}: fused step median {np.median(t_scalar):.3f} ms scalar mode, {np.median(t_col):.3f} ms per-column mode "
          f"({(np.median(t_col) / np.median(t_scalar) - 1) * 100:+.2f} %)")
    D.close()


if __name__ == "__main__":
    main()
