"""Multi-step runs without a GPU: the numpy dtype of the step schedule is elmk_run_step of include/elmk.h byte for byte (gcc's sizeof
and offsetof), and both builds export the entry points."""
import os
import re
import shutil
import subprocess

import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from tests.support import ROOT

HEADER = open(os.path.join(ROOT, "include", "elmk.h")).read()
MEMBERS = ("decday", "doy", "forc_slot", "forc_wt1", "forc_wt2", "month1", "month2", "month_wt1", "month_wt2")


def test_run_step_dtype_matches_the_c_struct(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "elmk.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(elmk_run_step));\n'
                   + "".join(f'  printf("{m} %zu\\n", offsetof(elmk_run_step, {m}));\n' for m in MEMBERS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out.pop("size")) == st.RUN_STEP_DTYPE.itemsize
    assert {k: int(v) for k, v in out.items()} == {m: st.RUN_STEP_DTYPE.fields[m][1] for m in MEMBERS}
    assert set(st.RUN_STEP_DTYPE.names) == set(MEMBERS)


def test_run_abi_is_declared_and_exported():
    flags = dict(re.findall(r"(ELMK_RUN_[A-Z_]+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in flags.items()} == {"ELMK_RUN_QBOT_IS_RH": st.RUN_QBOT_IS_RH, "ELMK_RUN_HISTORY": st.RUN_HISTORY}
    declared = {"elmk_run_reserve", "elmk_series_upload", "elmk_run", "elmk_run_diagnostics"}
    assert declared <= set(re.findall(r"^int (elmk_\w+)\(", HEADER, re.M))
    assert declared <= set(L.SIGNATURES)
    for path in (L.LIB_PATH, L.F32_LIB_PATH):
        lib = L.load(path)
        for name in declared:
            assert getattr(lib, name) is not None
