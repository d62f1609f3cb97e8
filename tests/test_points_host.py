"""The point series without a device (include/elmk.h "point series"): the numpy restatement against a straight loop, the ring's order,
the interface in every layer, and the kernel's text."""
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import points as pt
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from tests import output_map_cases as om
from tests import points_cases as pc

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ENTRY_POINTS = ("set", "add_field", "add_row", "add_cell_row", "add_gridded_field", "add_gridded_row", "reserve", "record", "set_run", "count",
                "read", "stamps", "reset", "clear")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_gather_restatement_equals_a_straight_loop():
    """Every stored type, the first and the last level of a field, -0.0, a NaN with a payload and both infinities: bit for bit."""
    rows = pc.synthetic_rows()
    ncols, ncells = rows["snl"].size, rows["VOLR"].size
    lists = (np.array([0, ncols - 1, 37, 37, 38, 74, 75, 111, 3]), np.array([ncells - 1, 0, 5, 5]))
    entries = [(name, pt.COLUMNS, pt.GATHER) for name in ("t_soisno/0", "t_soisno/last", "f32", "snl", "veg_active", "err_flags")]
    entries.append(("VOLR", pt.CELLS, pt.GATHER))
    got, want = pt.record(rows, lists, entries), pc.loop_record(rows, lists, entries)
    assert len(got) == len(entries)
    for (name, _, _), g, w in zip(entries, got, want):
        assert g.dtype == np.float64 and pc.same_bits(g, w), name
    # the specials arrived, as themselves
    v = got[0]  # (columns 0, 37, 74 and 111 hold the NaN, -0.0, +inf and -inf; one column on in the last level)
    assert np.isnan(v[0]) and pc.words(v[:1])[0] == pc.words(np.array([pc.NAN_PAYLOAD]))[0]
    assert pc.same_bits(v[2], -0.0) and pc.same_bits(v[2], v[3]) and v[5] == np.inf and v[7] == -np.inf
    assert pc.same_bits(got[1][4], -0.0) and got[1][6] == np.inf and np.isnan(got[2][0]) and pc.same_bits(got[2][2], -0.0)
    assert pc.same_bits(got[-1][:2], rows["VOLR"][[ncells - 1, 0]])
    assert got[5].max() > 2.0 ** 31 and (got[3] <= 0).all()  # uint32 above the int32 range, snl as signed


def test_gather_refuses_points_outside_the_row_and_other_types():
    rows = {"x": np.zeros(5)}
    for bad in ([5], [-1]):
        with pytest.raises(ValueError, match="outside the row"):
            pt.record(rows, (bad, []), [("x", pt.COLUMNS, pt.GATHER)])
    with pytest.raises(ValueError, match="stored element type"):
        pt.record({"x": np.zeros(5, np.int64)}, ([0], []), [("x", pt.COLUMNS, pt.GATHER)])
    with pytest.raises(ValueError, match="gridded entry"):
        pt.record(rows, ([0], [0]), [("x", pt.CELLS, pt.GRIDDED)])


@pytest.mark.parametrize("layout", ["tiles", "big_last"])
def test_gridded_restatement_equals_apply_aggregate(layout):
    """At the chosen cells bit for bit - a wide-range row with every edge value of output_map_cases at its place, an empty cell (fill)
    and a cell longer than a pass included - and, on finite values, equal to the straight loop."""
    ncells = 65
    lead, mid = om.edge_columns(ncells, layout)
    ptr, col, w, ncols = om.shape_map(ncells, 40, layout, lead=lead, mid=mid)
    cnt = np.diff(ptr)
    cells = np.array([int(np.argmax(cnt)), int(np.nonzero(cnt == 0)[0][0]), 0, ncells - 1, 5, 5])
    for seed, special in ((1, True), (2, False)):
        x = om.edge_values(ncols, seed, special=special)
        with np.errstate(invalid="ignore"):  # (0.0 * inf and inf - inf are among the edge values)
            (got,) = pt.record({"x": x}, ([], cells), [("x", pt.CELLS, pt.GRIDDED)], (ptr, col, w, om.FILL))
            want = RG.apply_aggregate(ptr, col, w, x, om.FILL)[cells]
        assert pc.same_bits(got, want) and got[1] == om.FILL
        if not special:
            (loop,) = pc.loop_record({"x": x}, ([], cells), [("x", pt.CELLS, pt.GRIDDED)], (ptr, col, w, om.FILL))
            assert pc.same_bits(got, loop)
    # a fp32-stored row is widened first
    x32 = om.edge_values(ncols, 3, span=30.0, special=False).astype(np.float32)
    (got,) = pt.record({"x": x32}, ([], cells), [("x", pt.CELLS, pt.GRIDDED)], (ptr, col, w, om.FILL))
    assert pc.same_bits(got, RG.apply_aggregate(ptr, col, w, x32.astype(np.float64), om.FILL)[cells])


def test_the_gpu_tests_map_has_the_shapes_it_names():
    ptr, col, w = pc.grid_map()
    cnt = np.diff(ptr)
    assert cnt[pc.BIG] == 2100 and cnt[pc.EXACT] == 64 and cnt[pc.EXACT1] == 65 and not cnt[list(pc.EMPTY)].any()
    assert col.min() >= 0 and col.max() < pc.NCOL and ptr.size == pc.NCELL_GRID + 1
    for n in pc.SIZES:
        a = pc.column_list(n)
        assert a.size == n and a.min() >= 0 and a.max() < pc.NCOL
    assert tuple(pc.column_list(65)[:6]) == pc.BASE_COLUMNS and pc.column_list(1)[0] == pc.NCOL - 1
    assert tuple(pc.cell_list(64)[:4]) == pc.BASE_CELLS and pc.cell_list(257).max() < pc.NCELL_ROWS


@pytest.mark.parametrize("total,records,slots", [(0, [], []), (1, [0], [0]), (4, [0, 1, 2, 3], [0, 1, 2, 3]), (5, [1, 2, 3, 4], [1, 2, 3, 0]),
                                                  (9, [5, 6, 7, 8], [1, 2, 3, 0])])
def test_ring_order(total, records, slots):
    r, s = pt.ring(total, 4)
    assert r.tolist() == records and s.tolist() == slots
    with pytest.raises(ValueError):
        pt.ring(total, 0)


def test_interface_in_every_layer():
    header, hpp = _read("include", "elmk.h"), _read("include", "elmk_interface.hpp")
    for name in ENTRY_POINTS:
        sym = "elmk_points_" + name
        assert sym in L.SIGNATURES, sym
        assert re.search(r"^int %s\(elmk_ctx \*ctx" % sym, header, re.M), sym
        assert callable(getattr(st.ELMState, "points_" + name)), name
        assert re.search(r"\b%s\(ctx_" % sym, hpp), sym
    assert "enum { ELMK_POINTS_COLUMNS = 0, ELMK_POINTS_CELLS = 1, ELMK_POINTS_NKIND = 2 };" in header
    assert "#define ELMK_POINTS_MAX_ENTRIES 64" in header and re.search(r"#define ELMK_POINTS_MAX_POINTS 4096\b", header)
    assert (pt.MAX_ENTRIES, pt.MAX_POINTS, pt.COLUMNS, pt.CELLS) == (64, 4096, 0, 1)
    assert "/* ---- point series ---" in header and all(f"P{k} " in header for k in range(10))
    # no run flag and no member of elmk_run_step: the struct and the flag list are what they were
    assert not re.search(r"#define ELMK_RUN_\w+ 512", header) and "points" not in re.search(r"typedef struct \{[^}]*\} elmk_run_step;", header, re.S).group(0)
    mk = _read("elmkernels_amd", "csrc", "Makefile")
    assert re.search(r"^KSRC\s*\+= k_points\.hip$", mk, re.M) and re.search(r"^HOSTSRC\s*\+= api_points\.cpp$", mk, re.M)
    assert mk.index("KSRC    += k_points.hip") < mk.index("OBJS    :=")  # both libraries' object lists take the new units


def test_kernel_text():
    """The record kernel shares nothing between threads: its unit names no read-modify-write, no fence and no cache hint, and the one
    launch serves the stepwise call and the run's step."""
    text = _read("elmkernels_amd", "csrc", "k_points.hip")
    for word in ("atomic", "__threadfence", "nontemporal", "__syncthreads"):
        assert word not in text, word
    assert text.count("__global__") == 1 and text.count("hipLaunchKernelGGL") == 1
    host = _read("elmkernels_amd", "csrc", "api_points.cpp")
    assert host.count("launch_points_record(") == 2  # the stepwise call and the run's stage
    run = _read("elmkernels_amd", "csrc", "api_run.cpp")
    assert re.search(r"\{run_history, nullptr\},\s*\{run_points, nullptr\},\s*\{run_next, nullptr\}", run)
