"""History tapes without a GPU: the C ABI of include/elmk.h ("history"), the ctypes table and the Python constants agree, and both
builds export the entry points."""
import os
import re

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from tests.support import ROOT

HEADER = open(os.path.join(ROOT, "include", "elmk.h")).read()


def test_history_abi_constants_match_the_header():
    ops = dict(re.findall(r"(ELMK_HIST_[A-Z]+) = (\d+)", HEADER))
    assert {k: int(v) for k, v in ops.items()} == {
        "ELMK_HIST_AVG": st.HIST_AVG, "ELMK_HIST_SUM": st.HIST_SUM, "ELMK_HIST_MAX": st.HIST_MAX, "ELMK_HIST_MIN": st.HIST_MIN,
        "ELMK_HIST_INST": st.HIST_INST}
    assert int(re.search(r"#define ELMK_HIST_MAX_TAPES (\d+)", HEADER).group(1)) == st.HIST_MAX_TAPES
    assert int(re.search(r"#define ELMK_HIST_MAX_ENTRIES (\d+)", HEADER).group(1)) == st.HIST_MAX_ENTRIES


def test_history_entry_points_are_declared_and_exported():
    declared = set(re.findall(r"^int (elmk_history_\w+)\(", HEADER, re.M))
    assert declared == {"elmk_history_add", "elmk_history_accumulate", "elmk_history_reset", "elmk_history_count",
                        "elmk_history_read", "elmk_history_clear"}
    assert declared <= set(L.SIGNATURES)
    for path in (L.LIB_PATH, L.F32_LIB_PATH):
        lib = L.load(path)  # declares every symbol of the table; raises if one is missing
        for name in declared:
            assert getattr(lib, name) is not None
