"""GPU: bench.py as a command, plain and with --full, once each at a small size.

A plain run prints the headline and the configuration and nothing that takes runs of its own; --full times the same steps
first and adds the rest to the line, so what the two leave in the state after the timed steps (--dump-outputs) is the
same bit for bit.

30 000 columns: more than the 24 064-column base block, so the state is tiled on the device as the benchmark's own is.
Two timed steps after one warm-up step: the fewest with a step that follows another.  --full runs without its 10 M-column
legs and without the CPU baseline, which are sized in seconds whatever --cols says."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS, STEPS, WARMUP = 30_000, 2, 1
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "device_state_GB", "dump_outputs"}
FULL_ONLY_KEYS = {"error_flags", "step_time", "roofline", "timestep_roofline", "kernels", "other_tier", "fused_step", "advance_step"}


def _bench(out_dir, *more):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--cols", str(COLS), "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--dump-outputs", str(out_dir)] + list(more)
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout.decode()  # ONE JSON line and nothing else on stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    return {"plain": _bench(d / "plain"), "full": _bench(d / "full", "--full", "--no-north-star", "--no-cpu-baseline"), "dir": d}


def _check_headline(line):
    assert line["metric"] == "gridcell-timesteps/sec" and line["unit"] == "gridcell-timesteps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["n_gpus"] == 1 and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["ms_per_step"] > 0 and abs(line["value"] - COLS / (line["ms_per_step"] * 1e-3)) < 1e-9 * line["value"]
    assert line["config"]["columns_per_gpu"] == COLS and line["config"]["tier"] == "fixture-tiled"


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_measured_beside_it(lines):
    line = lines["plain"]
    assert set(line) == PLAIN_KEYS, set(line) ^ PLAIN_KEYS
    _check_headline(line)


@pytest.mark.gpu
def test_full_run_adds_to_the_plain_line(lines):
    line = lines["full"]
    assert set(line) == PLAIN_KEYS | FULL_ONLY_KEYS, set(line) ^ (PLAIN_KEYS | FULL_ONLY_KEYS)
    _check_headline(line)
    from elmkernels_amd import state as st

    assert list(line["kernels"]) == list(st.KERNEL_NAMES) and all(k["ms"] > 0 for k in line["kernels"].values())
    assert line["step_time"]["n"] == 3 and 0 < line["step_time"]["min_ms"] <= line["step_time"]["median_ms"] <= line["step_time"]["max_ms"]
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["achieved"] > 0 and line["roofline"]["empirical_peak"] > 0
    assert line["other_tier"]["tier"] == "branch-mix" and line["other_tier"]["value"] > 0
    assert set(line["fused_step"]) == {"bytes_per_column_step", "fixture-tiled", "branch-mix"}
    assert isinstance(line["error_flags"], int)


@pytest.mark.gpu
def test_full_run_leaves_the_outputs_of_the_plain_run(lines):
    a, b = lines["dir"] / "plain", lines["dir"] / "full"
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and len(names) == lines["plain"]["dump_outputs"]["arrays"] > 100
    for name in names:
        assert np.array_equal(np.load(a / name), np.load(b / name), equal_nan=True), name
