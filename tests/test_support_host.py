"""The shared test modules (tests/support.py, tests/helpers.py): no test module imports another one, the two comparisons differ exactly
where they should, helpers keeps the names the benchmark and the tools import, and the state.bin writer keeps its bytes.  No GPU."""
import ast
import glob
import hashlib
import inspect
import os

import numpy as np

from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.support import ROOT, same, same_nan, state_blob


def _imported_test_modules(path):
    """The tests.test_* modules a source file imports, in any spelling."""
    found = []
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Import):
            found += [a.name for a in node.names if a.name.startswith("tests.test_")]
        elif isinstance(node, ast.ImportFrom):
            module = node.module or ""
            if module.startswith("tests.test_") or (node.level and module.startswith("test_")):
                found.append(module)
            elif module == "tests" or (node.level and not module):
                found += [a.name for a in node.names if a.name.startswith("test_")]
    return found


def test_no_module_imports_a_test_module():
    sources = glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True)
    assert len(sources) > 60
    offenders = {os.path.relpath(p, ROOT): m for p in sources if (m := _imported_test_modules(p))}
    assert not offenders, offenders


def test_same_and_same_nan_differ_where_they_should():
    a = np.array([1.0, -2.5, 0.0])
    assert same(a, a.copy()) and same_nan(a, a.copy())
    # the dtype only: the values are exact in both
    assert not same(a, a.astype(np.float32)) and same_nan(a, a.astype(np.float32))
    assert not same(np.array([1, 2], np.int32), np.array([1, 2], np.int64))
    # the payload of a NaN only
    quiet = np.array([0x7FF8000000000000, 0x3FF0000000000000], np.uint64).view(np.float64)
    other = np.array([0x7FF8000000000001, 0x3FF0000000000000], np.uint64).view(np.float64)
    assert np.isnan(quiet[0]) and np.isnan(other[0])
    assert not same(quiet, other) and same_nan(quiet, other)
    assert not same_nan(quiet, np.array([1.0, 1.0]))  # a NaN equals only a NaN
    # the sign of zero: different bits, and no NaN to excuse them
    assert not same(np.array([0.0]), np.array([-0.0])) and not same_nan(np.array([0.0]), np.array([-0.0]))
    # the shape
    assert not same(a, a.reshape(3, 1)) and not same_nan(a, a.reshape(3, 1))


def test_helpers_keeps_its_names_and_signatures():
    want = {"device_state": ["cols", "scal", "soil", "land", "device"], "oracle_state": ["cols", "scal", "soil", "land", "pft", "optics"],
            "compare_states": ["D", "S", "names", "rel", "skip_cols", "int_exact", "extra_scale", "bitwise"],
            "field_table_from_oracle": [], "field_floor": ["name", "extra_scale"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(H, name)).parameters)[:len(params)] == params, name
    for table in ("CANCEL_SCALE", "PHASE_CHANGE_SCALE"):
        assert isinstance(getattr(H, table), dict), table
    assert isinstance(H.LIBM_RESIDUAL_FIELDS, set) and H.REL_TOL == 1e-12 and H.ABS_FLOOR == 1e-18


def test_state_blob_keeps_the_bytes_of_the_writer_it_replaced():
    """A 3-column oracle state and the records of the run example (geography, two series, two steps).  The digest is that of the blob
    the writer inside tests/test_gpu_run.py::test_run_demo made for the same inputs in the commit before the writers were folded into
    support.state_blob (3e8e94b), computed on the CPU with that commit's code."""
    n = 3
    cols, scal, soil = synth.make_state(H.field_table_from_oracle(), n, tier="B", seed=74)
    lat, lon = synth.global_grid(n, seed=75)
    steps = np.zeros(2, st.RUN_STEP_DTYPE)
    steps["decday"] = [14.875, 14.895833333333334]
    steps["forc_slot"] = [0, 1]
    extra = [("lat", lat), ("lon", lon), ("series/atm_tbot", 280.0 + np.arange(2 * n, dtype=np.float64).reshape(2, n)),
             ("series/mlai", 0.5 * np.arange(12 * n, dtype=np.float64).reshape(12, n)), ("steps", steps)]
    blob = state_blob(H.oracle_state(cols, scal, soil), 1800.0, extra)
    assert len(blob) == 464171
    assert hashlib.sha256(blob).hexdigest() == "f5c0474b8771b7d9326c358a2fb15adc266d5e209963eae22528e60ffb36a496"
