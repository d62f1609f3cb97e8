"""Host: the measuring protocol of tests/tools/costlib.py - the schedules byte for byte from their formulas, the call sequence of the
timed regions on a stub context, the order of the turns, and the contexts compare_libraries opens, times and closes - and that every
cost tool imports without a device and without the built library."""
import glob
import importlib
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tests", "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)
import costlib as CL  # noqa: E402
from elmkernels_amd import state as st  # noqa: E402

NAMES = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_cost.py")) if not p.endswith("conservation_cost.py"))


def test_tools_import_without_device_or_library(tmp_path):
    assert len(NAMES) == 14
    code = "import sys, importlib\nsys.path.insert(0, sys.argv[1])\nfor n in sys.argv[2:]:\n    importlib.import_module(n)\nprint('imported', len(sys.argv) - 2)\n"
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, TOOLS] + NAMES, capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "imported 14", r.stderr[-2000:]


def test_shared_helpers_are_defined_once():
    """The copies are gone: each helper has one definition under tests/tools, and no tool flips the order or declares symbols itself."""
    sources = {p: open(p).read() for p in glob.glob(os.path.join(TOOLS, "*.py"))}
    for name in ("schedule(n)", "run_ms(", "back_to_back(", "spread(", "load_parent("):
        assert sum(("def " + name) in s for s in sources.values()) <= 1, name
    for p, s in sources.items():
        if not p.endswith("costlib.py"):
            assert "r % 2 == 0 else" not in s and "SIGNATURES" not in s, p


def test_schedule_from_its_formula():
    n = 6
    S = np.zeros(n, st.RUN_STEP_DTYPE)
    for s in range(n):
        ddoy = 180.25 + s * CL.DT / 86400.0
        S[s]["decday"] = ddoy + 1.0
        S[s]["doy"] = int(ddoy)
        S[s]["forc_slot"] = 0
        S[s]["forc_wt2"] = np.full(8, (s + 0.5) / n)
        S[s]["forc_wt1"] = 1.0 - np.full(8, (s + 0.5) / n)
        S[s]["month1"], S[s]["month2"] = 0, 1
        S[s]["month_wt1"], S[s]["month_wt2"] = 0.6, 0.4
    assert CL.DT == 1800.0
    assert CL.schedule(n).tobytes() == S.tobytes()


def _evolving(n, day0, slot, frac, months):
    S = np.zeros(n, st.RUN_STEP_DTYPE)
    for s in range(n):
        ddoy = day0 + s * 1800.0 / 86400.0
        S[s]["decday"], S[s]["doy"], S[s]["forc_slot"] = ddoy + 1.0, int(ddoy), slot(s)
        w2 = np.clip(frac(s) + 0.03 * np.arange(8), 0.0, 1.0)
        S[s]["forc_wt2"], S[s]["forc_wt1"] = w2, 1.0 - w2
        S[s]["month1"], S[s]["month2"] = months(s)
        S[s]["month_wt1"], S[s]["month_wt2"] = 0.4, 0.6
    return S


def test_evolving_schedules_from_their_constants():
    # shortwave_cost and downscaling_cost: 48 half-hour steps from day 171 over 3-hourly records, June into July
    want = _evolving(48, 171.0, lambda s: s // 6, lambda s: (s % 6) / 6, lambda s: (5, 6))
    for name in ("shortwave_cost", "downscaling_cost"):
        tool = importlib.import_module(name)
        assert (tool.NSTEPS, tool.SPR, tool.NREC, tool.DAY0) == (48, 6, 9, 171.0)
        assert tool.schedule().tobytes() == want.tobytes(), name
    # run_cost and forcing_grid_cost: hourly records from mid-January, the month bracket moving after 24 steps
    want = _evolving(48, 13.875, lambda s: s // 2, lambda s: (s % 2) * 0.5, lambda s: (11, 0) if s < 24 else (0, 1))
    for name in ("run_cost", "forcing_grid_cost"):
        assert importlib.import_module(name).schedule().tobytes() == want.tobytes(), name


class StubContext:
    """Records the calls a timed region makes; every run or launch takes one second on the stub clock."""

    def __init__(self, clock, name="ctx"):
        self.calls, self.clock, self.name, self.closed = [], clock, name, False

    def sync(self):
        self.calls.append("sync")

    def restore_fields(self):
        self.calls.append("restore_fields")

    def run(self, dt, steps, flags):
        self.calls.append(("run", dt, len(steps), flags))
        self.clock.t += 1.0

    def launch(self):
        self.calls.append("launch")
        self.clock.t += 1.0

    def close(self):
        self.closed = True


@pytest.fixture
def clock(monkeypatch):
    c = types.SimpleNamespace(t=100.0)
    monkeypatch.setattr(CL, "time", types.SimpleNamespace(perf_counter=lambda: c.t))
    return c


def test_run_ms_call_sequence(clock):
    D = StubContext(clock)
    steps = CL.schedule(4)
    ms = CL.run_ms(D, steps, 5)
    once = ["restore_fields", ("run", 1800.0, 4, 5)]
    assert D.calls == once + ["sync"] + once * 3 + ["sync"]
    assert ms == 3.0 / (3 * 4) * 1e3
    assert CL.run_ms(D, steps, 0, n=2) == 2.0 / (2 * 4) * 1e3


@pytest.mark.parametrize("n", [20, 40])
def test_back_to_back_call_sequence(clock, n):
    D = StubContext(clock)
    ms = CL.back_to_back(D, D.launch, n)
    assert D.calls == ["launch", "sync"] + ["launch"] * n + ["sync"]
    assert ms == float(n) / n * 1e3


def test_wall_ms_call_sequence(clock):
    D = StubContext(clock)
    assert CL.wall_ms(D, D.launch) == 1e3 and D.calls == ["sync", "launch"]
    assert CL.wall_ms(D, D.launch, sync_after=True) == 1e3 and D.calls == ["sync", "launch"] * 2 + ["sync"]


def test_interleave_and_spread():
    keys = ("a", "b", "c")
    assert [CL.interleave(r, keys) for r in range(4)] == [["a", "b", "c"], ["c", "b", "a"]] * 2
    assert CL.interleave(1, {"x": 1, "y": 2}) == ["y", "x"]
    assert CL.spread([1, 2, 4]) == 1.5
    res = {"a": [1.0, 2.0, 4.0], "b": [3.0, 3.0]}
    assert CL.medians(res) == {"a": 2.0, "b": 3.0} and CL.spreads(res) == {"a": 1.5, "b": 0.0}


@pytest.mark.parametrize("first,parent2", [(None, False), ("this", False), ("parent", False), ("parent", True), (None, True)])
def test_compare_libraries(clock, monkeypatch, first, parent2):
    loaded, built, turns = [], [], []
    monkeypatch.setattr(CL, "load_build", lambda path, optional=(): loaded.append((path, optional)))
    libs = [("this", None), ("parent", "p.so")] + ([("parent2", "p2.so")] if parent2 else [])
    cost = {None: 1.0, "p.so": 2.0, "p2.so": 3.0}

    def build(cols, path):
        D = StubContext(clock, path)
        built.append(D)
        return D

    def time_one(D):
        turns.append(D.name)
        return cost[D.name]

    rounds = 4
    out = CL.compare_libraries(1000, rounds, libs, build, time_one, first=first, optional=("elmk_new_",), baseline="parent")
    names = [p for _, p in libs]
    assert loaded == [(p, ("elmk_new_",)) for p in names if p]
    assert [D.name for D in built] == (["p.so"] + [p for p in names if p != "p.so"] if first == "parent" else names)
    assert turns == (names + names[::-1]) * (rounds // 2)
    assert all(D.closed for D in built) and len(built) == len(libs)
    assert out["all"] == {k: [cost[p]] * rounds for k, p in libs}
    assert out["median"] == {k: cost[p] for k, p in libs} and out["spread"] == {k: 0.0 for k, _ in libs}
    assert out["this_over_parent"] == 0.5
    assert (out["parent2_over_parent"] == 1.5) if parent2 else ("parent2_over_parent" not in out)
    assert set(out) == {"all", "median", "spread", "this_over_parent"} | ({"parent2_over_parent"} if parent2 else set())


def test_compare_libraries_modes_and_failure(clock, monkeypatch):
    monkeypatch.setattr(CL, "load_build", lambda path, optional=(): None)
    built, turns = [], []

    def build(cols, path):
        built.append(StubContext(clock, path))
        return built[-1]

    modes = {m: (lambda D, m=m: turns.append((m, D.name)) or 1.0) for m in ("x", "y")}
    prepared = []
    out = CL.compare_libraries(8, 2, [("product", None), ("variant", "v.so")], build, modes, prepare=lambda ctx: prepared.append(list(ctx)))
    assert prepared == [["product", "variant"]]
    assert turns == [("x", None), ("x", "v.so"), ("y", None), ("y", "v.so"), ("x", "v.so"), ("x", None), ("y", "v.so"), ("y", None)]
    assert out["all"] == {k: {"x": [1.0, 1.0], "y": [1.0, 1.0]} for k in ("product", "variant")}
    assert set(out) == {"all", "median", "spread"}
    # a timed region that raises still leaves no context open
    del built[:]
    with pytest.raises(ZeroDivisionError):
        CL.compare_libraries(8, 2, [("this", None), ("parent", "p.so")], build, lambda D: 1 / 0)
    assert len(built) == 2 and all(D.closed for D in built)
