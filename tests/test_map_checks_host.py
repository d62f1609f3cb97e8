"""The host checks of the ELL and CSR maps (elmkernels_amd/csrc/elmk_maps.h) without a GPU: tests/c/map_checks.cc includes only that
header, runs one case per line and prints what the check returned.  Every expected text is the message elmk_set_forcing_grid,
elmk_aerosol_reserve, elmk_set_output_grid and elmk_set_downscaling_groups give behind their own name (the GPU tests' refusals pin
the names).  These checks are what keeps the map kernels' gathers inside their buffers."""
import os
import subprocess
import warnings

import pytest

from tests.support import ROOT


NPTS = "npts outside 1 .. 8"
NCELLS = "ncells outside 1 .. 2^31-1"
NGROUPS = "ngroups outside 1 .. 2^31-1"
NULL_MAP = "null map"
IDX0 = "idx[0] outside [0, ncells)"
IDX = "idx outside [-1, ncells)"
WEIGHT = "non-finite weight"
COL = "col outside [0, ncols)"
TWICE = "a column in more than one group (or twice in one)"
WEIGHT_GE0 = "weight not finite and >= 0"

EXPECTED = [(f"ell_npad({n})", str(p)) for n, p in zip(range(1, 9), (1, 2, 4, 4, 8, 8, 8, 8))] + [
    ("ell npts 0", NPTS),
    ("ell npts 9", NPTS),
    ("ell ncells 0", NCELLS),
    ("ell ncells 2^31", NCELLS),
    ("ell null idx", NULL_MAP),
    ("ell null w", NULL_MAP),
    ("ell idx[0] -1", IDX0),
    ("ell idx[0] ncells", IDX0),
    ("ell idx[1] -2", IDX),
    ("ell idx[1] ncells", IDX),
    ("ell NaN weight", WEIGHT),
    ("ell inf weight", WEIGHT),
    ("ell NaN behind padding", "ok"),
    ("ell no columns", "ok"),
    ("ell valid 1", "ok"),
    ("ell valid 2", "ok"),
    ("ell valid 3", "ok"),
    ("ell valid 8", "ok"),
    # rows outer, columns inner, per entry the index before the weight; the arguments before the map, npts first
    ("ell bad weight in row 0, bad idx in row 1", WEIGHT),
    ("ell bad idx and bad weight in one row", WEIGHT),
    ("ell npts 0 and ncells 0", NPTS),
    ("csr nrows 0, cells", NCELLS),
    ("csr nrows 0, groups", NGROUPS),
    ("csr null ptr", "null ptr"),
    ("csr ptr[0] 1", "ptr[0] != 0"),
    ("csr ptr decreasing", "ptr decreasing"),
    ("csr nnz 2^31", "nnz outside 0 .. 2^31-1"),  # (from ptr alone: col and w are null and never read)
    ("csr null col", NULL_MAP),
    ("csr null w", NULL_MAP),
    ("csr col -1", COL),
    ("csr col ncols", COL),
    ("csr repeated column, unique", TWICE),
    ("csr repeated column, repeats allowed", "ok"),
    ("csr NaN weight, cells", WEIGHT),
    ("csr NaN weight, groups", WEIGHT_GE0),
    ("csr weight -1, non-negative", WEIGHT_GE0),
    ("csr weight -1, finite only", "ok"),
    ("csr empty rows", "ok"),
    ("csr nnz 0", "ok"),
    # per term: the column's range, then uniqueness, then the weight
    ("csr repeated column with a bad weight", TWICE),
    ("csr bad column with a bad weight", COL),
]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    """The program's output; built with the address and undefined-behaviour sanitizers where the host compiler links their static
    runtimes (an out-of-range read of a map then ends the program), else without."""
    exe = str(tmp_path_factory.mktemp("map_checks") / "map_checks")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "map_checks.cc"), "-o", exe]
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd + san, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    sanitized = r.returncode == 0
    if not sanitized:  # (said aloud: without the sanitizers an out-of-range read of a map may pass unseen)
        warnings.warn("map_checks.cc built WITHOUT -fsanitize=address,undefined: the host compiler does not link them here:\n"
                      + r.stderr.decode()[-400:])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    print("map_checks.cc built", "with" if sanitized else "without", "-fsanitize=address,undefined")
    # (the program's vectors are all freed; leak detection needs ptrace, which a container may deny)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().splitlines()


def test_every_case_returns_the_entry_points_message(lines):
    got = [tuple(s.split(": ", 1)) for s in lines]
    assert got == EXPECTED


def test_the_header_needs_no_hip_and_no_context():
    text = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "elmk_maps.h")).read()
    includes = [s.split()[1] for s in text.splitlines() if s.startswith("#include")]
    assert sorted(includes) == ["<cmath>", "<cstdint>", "<vector>"]
    assert "elmk_ctx" not in text
