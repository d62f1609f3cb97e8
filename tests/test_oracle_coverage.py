"""Line coverage of the oracle's physics by the parity case list (tests/parity_cases.py).

The oracle is built with gcc --coverage in a temporary directory and the whole case list is replayed through it in a child
Python (ELMO_LIBRARY selects that build).  Every executable line of the physics files must have run, except lines an explicit
marker in the oracle source names as unreached, with its reason:

    /* unreached: <reason> */

A marker covers the line it stands on; a marker alone on a line covers the next line.  If the covered line opens a block
(its code ends with "{"), the block is covered too, up to the first "}" at that line's indentation.  Reasons are: unreachable by construction, reached
only by another named test, or a throw site of the reference (tests/test_gpu_parity.py::test_error_flags_match_the_reference_
throw_sites and tests/test_oracle_vs_ref_canopy.py cover those).  A branch the case list reaches is therefore one the device
parity tests run against the oracle; a branch it does not reach must be named here, never silently untested.
Per-file line and branch figures are printed (pytest -s shows them)."""
import glob
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

from tests.support import ROOT

ORACLE = os.path.join(ROOT, "oracle")
SRCS = ["elmo_physics_a.c", "elmo_physics_b.c", "elmo_physics_c.c", "elmo_physics_d.c", "elmo_physics_e.c", "elmo_physics_f.c",
        "elmo_physics_g.c", "elmo_physics_h.c", "elmo_driver.c"]
CHECKED = ["elmo_physics_a.c", "elmo_physics_b.c", "elmo_physics_c.c", "elmo_physics_d.c", "elmo_physics_e.c", "elmo_physics_g.c"]
MARKER = re.compile(r"/\*\s*unreached:\s*(.*?)\s*\*/")

REPLAY = r"""
import sys
from tests import parity_cases as P
names = sys.argv[1:]
for c in P.CASES:
    if not names or c.name in names:
        P.replay(c)
print("replayed", len(P.CASES))
"""


def _code(line):
    """The line without comments (block comments on one line, and a trailing // comment)."""
    return re.sub(r"//.*$", "", re.sub(r"/\*.*?\*/", "", line)).strip()


def marked_lines_of(lines, i):
    """-> {line number (1-based): reason} of the lines the marker on line i (0-based) covers."""
    reason = MARKER.search(lines[i]).group(1)
    assert len(reason) >= 10, f"line {i + 1}: an unreached marker needs its reason"
    covered = {}
    j = i
    if not _code(lines[i]):  # marker on its own line: it covers the next line of code
        j = i + 1
        while j < len(lines) and not _code(lines[j]):
            j += 1
    covered[j + 1] = reason
    if j + 1 < len(lines) and _code(lines[j + 1]) == "{":  # a function: its brace stands on the next line
        j += 1
        covered[j + 1] = reason
    if _code(lines[j]).endswith("{"):  # a block: up to the first "}" at the opening line's indentation
        indent = len(lines[j]) - len(lines[j].lstrip())
        for k in range(j + 1, len(lines)):
            covered[k + 1] = reason
            if _code(lines[k]).startswith("}") and len(lines[k]) - len(lines[k].lstrip()) == indent:
                break
    return covered


def marked_lines(path):
    """-> {line number (1-based): reason} of every line a marker covers; raises on a marker without a reason."""
    lines = open(path).read().split("\n")
    covered = {}
    for i, line in enumerate(lines):
        if MARKER.search(line):
            covered.update(marked_lines_of(lines, i))
    return covered


def coverage(names=None, keep=None):
    """Build the oracle with --coverage, replay the cases (all, or those named), -> {file: gcov json of the file}."""
    d = keep or tempfile.mkdtemp()
    try:
        objs = []
        for s in SRCS:
            o = os.path.join(d, s[:-2] + ".o")
            subprocess.check_call(["gcc", "-O0", "-std=c99", "-fPIC", "-fopenmp", "-ffp-contract=off", "-fno-fast-math", "--coverage",
                                   "-fprofile-update=atomic", "-c", os.path.join(ORACLE, s), "-o", o], cwd=d)
            objs.append(o)
        lib = os.path.join(d, "libelmoracle_cov.so")
        subprocess.check_call(["gcc", "-shared", "--coverage", "-fopenmp", "-o", lib] + objs + ["-lm"], cwd=d)
        env = dict(os.environ, ELMO_LIBRARY=lib, OMP_NUM_THREADS="4",
                   PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        r = subprocess.run([sys.executable, "-c", REPLAY] + list(names or []), cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=1200)
        assert r.returncode == 0 and "replayed" in r.stdout, r.stderr[-3000:]
        subprocess.check_call(["gcov", "-b", "-j", "-o", d] + [os.path.join(ORACLE, s) for s in CHECKED], cwd=d,
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out = {}
        for f in glob.glob(os.path.join(d, "*.gcov.json.gz")):
            for entry in json.load(gzip.open(f))["files"]:
                name = os.path.basename(entry["file"])
                if name in CHECKED:
                    out[name] = entry
        return out
    finally:
        if keep is None:
            shutil.rmtree(d, ignore_errors=True)


def report(cov):
    """-> ({file: [uncovered, unmarked line numbers]}, table text with the per-file figures)."""
    missing = {}
    rows = [f"{'file':<20} {'lines run':>14} {'branch outcomes taken':>22} {'unreached (marked)':>19}"]
    for name in CHECKED:
        marks = marked_lines(os.path.join(ORACLE, name))
        lines = cov[name]["lines"]
        run = sum(1 for ln in lines if ln["count"] > 0)
        br = [b for ln in lines for b in ln["branches"]]
        taken = sum(1 for b in br if b["count"] > 0)
        unrun = [ln["line_number"] for ln in lines if ln["count"] == 0]
        missing[name] = [k for k in unrun if k not in marks]
        marked = sum(1 for k in unrun if k in marks)
        rows.append(f"{name:<20} {run:>6}/{len(lines):<5} {100.0 * run / len(lines):5.1f}% {taken:>7}/{len(br):<5} "
                    f"{100.0 * taken / max(1, len(br)):5.1f}% {marked:>10}")
    return missing, "\n".join(rows)


@pytest.mark.skipif(shutil.which("gcc") is None or shutil.which("gcov") is None, reason="no gcc / gcov")
def test_every_oracle_line_is_run_by_the_parity_cases_or_marked_unreached():
    cov = coverage()
    missing, table = report(cov)
    print("\noracle coverage by tests/parity_cases.py:\n" + table)
    bad = {k: v for k, v in missing.items() if v}
    assert not bad, f"oracle lines no parity case runs and no 'unreached:' marker explains: {bad}\n{table}"


def test_markers_carry_reasons_and_cover_code():
    """Every marker in the checked files names its reason and covers at least one line of code of its own."""
    for name in CHECKED:
        path = os.path.join(ORACLE, name)
        src = open(path).read().split("\n")
        for i, line in enumerate(src):
            if MARKER.search(line):
                one = marked_lines_of(src, i)
                assert one and any(_code(src[k - 1]) for k in one), f"{name}:{i + 1}: marker covers no code"
