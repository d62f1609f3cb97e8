"""GPU: every tests/tools/*_cost.py tool, every mode, once at the smallest size - the record each mode emits has the key structure of
tests/cost_tool_keys.json (recorded from the tools as they stood before they were rewritten on tests/tools/costlib.py, with the cases of
CASES below), every timing in it is finite and positive, and every context the tool created is closed again.  Timings are not
compared at this size.

4096 columns: the smallest count in a tool's own defaults (run_cost).  Two rounds: the fewest in which the order of the turns flips.
Two run steps: the fewest with a step that follows another; run_cost, shortwave_cost and downscaling_cost keep their own 48.  A copy of
libelmk.so under another file name stands in for the other build of every comparison mode."""
import importlib
import json
import math
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tests", "tools")
KEYS = os.path.join(ROOT, "tests", "cost_tool_keys.json")
COLS, ROUNDS, STEPS, THREADS = 4096, 2, 2, 4

# tool -> (label, function, arguments); "LIB" and "LIB2" are the stand-in builds, "HIP" restart_cost's handle of the HIP runtime
CASES = {
    "accum_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("ab", "ab", (COLS, ROUNDS, STEPS, "LIB"))],
    "active_layer_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("ab", "ab", (COLS, ROUNDS, STEPS, "LIB")),
                          ("parent", "parent", (COLS, ROUNDS, STEPS, "LIB", False)),
                          ("parent_first", "parent", (COLS, ROUNDS, STEPS, "LIB", True))],
    "aerosol_cost": [("measure", "measure", (COLS, ROUNDS, STEPS, None)), ("parent_lib", "measure", (COLS, ROUNDS, STEPS, "LIB"))],
    "downscaling_cost": [("measure", "measure", (COLS, ROUNDS, ["off", "topo", "topo_groups"])),
                         ("only", "measure", (COLS, ROUNDS, ["topo_groups"]))],
    "forcing_grid_cost": [("measure", "measure", (COLS, ROUNDS, THREADS)),
                          ("only", "measure", (COLS, ROUNDS, THREADS, "column/spatial")),
                          ("ab", "measure", (COLS, ROUNDS, THREADS, "grid/16/bilinear/shuffled", "LIB"))],
    "frost_table_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("parent", "parent", (COLS, ROUNDS, "LIB", False)),
                         ("parent_first", "parent", (COLS, ROUNDS, "LIB", True))],
    "history_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("ab", "ab", (COLS, ROUNDS, "LIB"))],
    "hydrology_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("parent", "parent", (COLS, ROUNDS, STEPS, "LIB", False)),
                       ("parent_first", "parent", (COLS, ROUNDS, STEPS, "LIB", True))],
    "irrigation_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("parent", "parent", (COLS, ROUNDS, STEPS, "LIB", False)),
                        ("parent_first_parent2", "parent", (COLS, ROUNDS, STEPS, "LIB", True, "LIB2"))],
    "output_grid_cost": [("measure", "measure", (COLS, ROUNDS, STEPS))],
    "restart_cost": [("measure", "measure", (COLS, ROUNDS, "HIP"))],
    "run_cost": [("measure", "measure", (COLS, ROUNDS))],
    "shortwave_cost": [("measure", "measure", (COLS, ROUNDS, ["reference", "coszen"])), ("only", "measure", (COLS, ROUNDS, ["coszen"]))],
    "water_balance_cost": [("measure", "measure", (COLS, ROUNDS, STEPS)), ("store_ab", "store_ab", (COLS, ROUNDS, "LIB")),
                           ("parent", "parent", (COLS, ROUNDS, STEPS, "LIB", None)),
                           ("parent2", "parent", (COLS, ROUNDS, STEPS, "LIB", "LIB2"))],
}

# a number below one of these keys is a timing; the named ones are differences of two timings and may have either sign
TIMING_KEY = re.compile(r"(^|_)(all|median)$|_ms$")
DIFFERENCES = {"run_step_added_ms", "run_minus_parent_ms", "parent_spread_ms", "run_step_wb_added_ms", "run_step_4_entries_added_ms"}


def stand_ins(directory):
    """Two copies of the built library under other file names."""
    from elmkernels_amd import _lib as L

    out = {}
    for key, name in (("LIB", "libelmk_other.so"), ("LIB2", "libelmk_other2.so")):
        out[key] = shutil.copy(L.LIB_PATH, os.path.join(str(directory), name))
    return out


def run_cases(tool, libs, tools_dir=TOOLS):
    """{label: record} of the tool's cases, every record as it comes back from a JSON line."""
    if tools_dir not in sys.path:
        sys.path.insert(0, tools_dir)
    mod = importlib.import_module(tool)
    assert os.path.dirname(os.path.abspath(mod.__file__)) == os.path.abspath(tools_dir)
    out = {}
    for label, fn, args in CASES[tool]:
        args = [mod.hip_runtime() if a == "HIP" else libs.get(a, a) if isinstance(a, str) else a for a in args]
        out[label] = json.loads(json.dumps(getattr(mod, fn)(*args)))
    return out


def structure(x):
    """Keys, recursively; a list keeps its length (one entry per element); a leaf keeps its kind."""
    if isinstance(x, dict):
        return {k: structure(v) for k, v in x.items()}
    if isinstance(x, list):
        return [structure(v) for v in x]
    return "bool" if isinstance(x, bool) else "number" if isinstance(x, (int, float)) else "null" if x is None else "str"


def numbers(x, timing=False):
    """(number, is it a timing) of every numeric leaf."""
    if isinstance(x, dict):
        for k, v in x.items():
            yield from numbers(v, (timing or bool(TIMING_KEY.search(k))) and k not in DIFFERENCES)
    elif isinstance(x, list):
        for v in x:
            yield from numbers(v, timing)
    elif isinstance(x, (int, float)) and not isinstance(x, bool):
        yield x, timing


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return stand_ins(tmp_path_factory.mktemp("builds"))


@pytest.fixture(scope="module")
def table():
    with open(KEYS) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("tool", sorted(CASES))
def test_cost_tool(tool, libs, table, monkeypatch):
    from elmkernels_amd import state as st

    live = set()
    create, close = st.ELMState.__init__, st.ELMState.close

    def counted_create(self, *a, **kw):
        create(self, *a, **kw)
        live.add(id(self))

    def counted_close(self):
        close(self)
        live.discard(id(self))

    monkeypatch.setattr(st.ELMState, "__init__", counted_create)
    monkeypatch.setattr(st.ELMState, "close", counted_close)
    records = run_cases(tool, libs)
    assert not live, f"{len(live)} contexts left open"
    assert set(records) == set(table[tool])
    for label, rec in records.items():
        assert structure(rec) == table[tool][label], label
        ntimings = 0
        for v, timing in numbers(rec):
            assert math.isfinite(v), (label, v)
            if timing:
                assert v > 0.0, (label, v)
                ntimings += 1
        assert ntimings >= ROUNDS, label
