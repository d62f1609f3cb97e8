"""Cell rows on history tapes and the routing state in the image, without a GPU: the numpy fold against a scalar reading of the header's
"history" paragraph on rows with NaN, +-inf, -0.0 and subnormals; restart.py on hand-assembled images - a cell-row entry, a version-6
image with the routing's call count and cell sections checksummed with g = the cell, what merge and slice refuse, and images without the
new kinds, which parse and rebuild byte for byte as before; the header's constants and the bindings."""
import math
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import history as hs
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests.support import ROOT

NAN, INF = float("nan"), float("inf")
EDGE = (0.0, -0.0, 5e-324, -5e-324, 2.2250738585072009e-308, 1e300, -1e300, 1.7976931348623157e308, INF, -INF, NAN, 1.5, -3.5e4)


def _words(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64("nan"), a).view(np.uint64)  # (which NaN: the one thing IEEE leaves open)


def _scalar_fold(op, samples):
    """The header's paragraph read literally, one cell, Python floats."""
    acc = {"avg": -0.0, "sum": -0.0, "max": -INF, "min": INF, "inst": NAN}[op]
    for v in samples:
        if op in ("avg", "sum"):
            acc = acc + v
        elif op == "max":
            acc = v if (v > acc or v != v) else acc
        elif op == "min":
            acc = v if (v < acc or v != v) else acc
        else:
            acc = v
    return acc / float(len(samples)) if op == "avg" else acc


def _edge_samples(nsteps, seed):
    """[nsteps] rows in which every pair of EDGE values meets in every order, beside ordinary values."""
    rng = np.random.default_rng(seed)
    pairs = np.array([(a, b) for a in EDGE for b in EDGE])
    n = len(pairs) + 50
    rows = []
    for k in range(nsteps):
        r = rng.normal(0.0, 1.0e3, n)
        r[:len(pairs)] = pairs[:, k % 2] if k < 2 else (pairs[:, 0] if k == 3 else rng.choice(EDGE, len(pairs)))
        rows.append(r)
    return rows


@pytest.mark.parametrize("op", ["avg", "sum", "max", "min", "inst"])
def test_the_numpy_fold_is_the_header_paragraph(op):
    rows = _edge_samples(5, 17)
    got = hs.fold_cell_rows(op, rows)
    want = np.array([_scalar_fold(op, [float(r[c]) for r in rows]) for c in range(rows[0].size)])
    assert (_words(got) == _words(want)).all(), np.nonzero(_words(got) != _words(want))[0][:5]
    # the code is the name's; AVG is the raw sum divided once
    assert (_words(hs.fold_cell_rows(hs.OPS[op], rows)) == _words(got)).all()
    raw = hs.fold_cell_rows(op, rows, raw=True)
    with np.errstate(all="ignore"):
        assert (_words(raw / 5.0 if op == "avg" else raw) == _words(got)).all()


def test_the_fold_keeps_signed_zeros_nans_and_subnormals():
    z = np.array([-0.0])
    assert math.copysign(1.0, hs.fold_cell_rows("sum", [z, z])[0]) == -1.0  # from -0.0: the exact additive identity
    assert math.copysign(1.0, hs.fold_cell_rows("sum", [z, -z])[0]) == 1.0
    assert math.copysign(1.0, hs.fold_cell_rows("avg", [z])[0]) == -1.0
    assert hs.fold_cell_rows("sum", [np.array([5e-324]), np.array([5e-324])])[0] == 1e-323
    for op in ("max", "min"):  # a NaN sticks, wherever it comes
        for k in range(3):
            rows = [np.array([1.0]), np.array([2.0]), np.array([-7.0])]
            rows[k] = np.array([NAN])
            assert np.isnan(hs.fold_cell_rows(op, rows)[0]), (op, k)
    assert hs.fold_cell_rows("max", [np.array([-INF])])[0] == -INF and hs.fold_cell_rows("min", [np.array([INF])])[0] == INF
    assert hs.fold_cell_rows("inst", [np.array([NAN]), np.array([3.0])])[0] == 3.0
    assert np.isnan(hs.init_value("inst")) and math.copysign(1.0, hs.init_value("avg")) == -1.0
    with pytest.raises(ValueError):
        hs.fold_cell_rows("avg", [])
    with pytest.raises(ValueError):
        hs.fold_cell_rows("avg", [np.zeros(3), np.zeros(4)])
    with pytest.raises(ValueError):
        hs.fold(9, np.zeros(1), np.zeros(1))


# ---- restart.py on hand-assembled images ----------------------------------------------------------------------------------------------
NCOL, NCELL, GCOL0 = 23, 9, 1000


def _image(cell_entry=False, routing=(), irrsup=False, ncalls=4, kinds_before=(R.IRRIGATION_SECTION,)):
    """Two field sections, a column history entry, optionally a cell-row entry (gridded = 2) with its GRIDDED section, the column kinds
    of kinds_before, then the cell sections of version 6: -> (image, the data per section)."""
    rng = np.random.default_rng(5)
    h = np.zeros((), R.HEADER)
    h["magic"], h["real_bytes"], h["schema_hash"], h["gcol0"], h["ncols"] = R.MAGIC, 8, 77, GCOL0, NCOL
    h["tape_count"][:2] = (3, 3)
    ent = [(0, 4, st.HIST_AVG, 0, 0)]
    secs = [(R.FIELD, 4, 1, 0, NCOL), (R.FIELD, 7, 2, 1, NCOL), (R.HISTORY, 0, 1, 0, NCOL)]
    if cell_entry:
        ent.append((1, R.row_field(R.ROWS_NFAMILY + R.CELL_ROWS_ROUTING, rt.QOUT), st.HIST_MAX, R.CELL_ROW_ENTRY, NCELL))
        secs.append((R.GRIDDED, 1, 1, 0, NCELL))
    secs += [(k, i, 1, 0, NCOL) for k in kinds_before for i in range(2)]
    secs += [(R.ROUTING_SECTION, w, 1, 0, NCELL) for w in routing]
    if irrsup:
        secs.append((R.IRRSUP_SECTION, ir.UNMET_SUM, 1, 0, NCELL))
    sec = np.zeros(len(secs), R.SECTION)
    data = []
    for i, (kind, sid, nlev, dt, ext) in enumerate(secs):
        d = (rng.integers(0, 6, (nlev, ext)) if dt else rng.standard_normal((nlev, ext))).astype(R.ELEM[dt])
        sec[i] = (kind, sid, nlev, dt, ext, 0, R.checksum(d, 0 if kind in R.CELL_SECTIONS else GCOL0))
        data.append(d)
    return R.build(h, np.array(ent, R.ENTRY), sec, data, routing_ncalls=ncalls), data


ROUTE_IDS = (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF)


def test_a_version_6_image_parses_and_verifies():
    img, data = _image(cell_entry=True, routing=ROUTE_IDS, irrsup=True, ncalls=4)
    p = R.verify(img)
    assert int(p["header"]["version"]) == R.VERSION_ROUTING == 6 and p["routing_ncalls"] == 4
    # the two words after the header: the accumulator count (0) and the call count
    assert np.frombuffer(img[R.HEADER.itemsize:R.HEADER.itemsize + 16].tobytes(), "<i8").tolist() == [0, 4]
    kinds = [int(s["kind"]) for s in p["sections"]]
    assert kinds[-6:] == [R.ROUTING_SECTION] * 5 + [R.IRRSUP_SECTION] and [int(s["id"]) for s in p["sections"][-6:]] == list(ROUTE_IDS) + [ir.UNMET_SUM]
    for s, d, want in zip(p["sections"], p["data"], data):
        assert d.tobytes() == want.tobytes()
        if int(s["kind"]) in R.CELL_SECTIONS:  # g = the cell: the checksum does not know gcol0
            assert int(s["extent"]) == NCELL and int(s["checksum"]) == R.checksum(want, 0) != R.checksum(want, GCOL0)
        else:
            assert int(s["checksum"]) == R.checksum(want, GCOL0)
    assert int(p["entries"][1]["gridded"]) == R.CELL_ROW_ENTRY == 2 and int(p["entries"][1]["ncells"]) == NCELL
    assert R.entry_row(p["entries"][1]["field"]) == (R.ROWS_NFAMILY + R.CELL_ROWS_ROUTING, rt.QOUT) == (5, 2)
    assert R.entry_row(p["entries"][1]["field"])[0] >= R.ROWS_NFAMILY  # no column family reaches it
    # the linear scheme alone, no limit: still version 6
    lin, _ = _image(routing=ROUTE_IDS[:2], ncalls=0)
    q = R.verify(lin)
    assert int(q["header"]["version"]) == 6 and q["routing_ncalls"] == 0 and lin.size < img.size


def test_damage_to_a_version_6_image_is_found():
    img, _ = _image(routing=ROUTE_IDS[:2], ncalls=7)
    p = R.parse(img)
    volr = next(i for i, s in enumerate(p["sections"]) if int(s["kind"]) == R.ROUTING_SECTION)
    flipped = img.copy()
    flipped[int(p["sections"][volr]["offset"]) + 11] ^= 4
    with pytest.raises(R.RestartError, match="section checksum mismatch .kind 7, id 0"):
        R.verify(flipped)
    count = img.copy()
    count[R.HEADER.itemsize + 8] ^= 1  # the call count is under the header checksum
    with pytest.raises(R.RestartError, match="header checksum"):
        R.verify(count)
    older = img.copy()
    older[8:12] = np.frombuffer(np.array([5], "<u4").tobytes(), np.uint8)  # version 5 with the sections of version 6
    with pytest.raises(R.RestartError):
        R.parse(older)
    newer = img.copy()
    newer[8:12] = np.frombuffer(np.array([7], "<u4").tobytes(), np.uint8)
    with pytest.raises(R.RestartError, match="format version"):
        R.parse(newer)
    with pytest.raises(R.RestartError, match="truncated"):
        R.parse(img[:R.HEADER.itemsize + 12])


def test_merge_and_slice_refuse_cell_data():
    v6, _ = _image(routing=ROUTE_IDS[:2])
    entry, _ = _image(cell_entry=True)
    assert int(R.verify(entry)["header"]["version"]) == R.VERSION_IRRIGATION  # a cell-row entry changes no version
    for img, text in ((v6, "version-6 image holds the routing state"), (entry, "cell-row history entries")):
        with pytest.raises(R.RestartError, match="merge: .*" + text):
            R.merge([img])
        with pytest.raises(R.RestartError, match="slice: .*" + text):
            R.slice(img, GCOL0, 5)


def test_images_without_the_new_kinds_are_what_they_were():
    """Versions 1 and 5 built by hand: one count word or none, no call count, parse, slice and merge as before, and the bytes of a
    rebuild; OPTIONAL, the column kinds, is the tuple it was."""
    for kinds, version, word in (((), 1, 0), ((R.IRRIGATION_SECTION,), 5, 8)):
        img, data = _image(kinds_before=kinds)
        p = R.verify(img)
        assert int(p["header"]["version"]) == version and p["routing_ncalls"] is None
        first = R.HEADER.itemsize + word
        assert np.frombuffer(img[first:first + R.ENTRY.itemsize].tobytes(), R.ENTRY)[0]["field"] == 4  # the entry table follows at once
        assert R.build(p["header"], p["entries"], p["sections"], p["data"], p["accum"]).tobytes() == img.tobytes()
        parts = [R.slice(img, GCOL0, 10), R.slice(img, GCOL0 + 10, NCOL - 10)]
        assert R.merge(parts[::-1]).tobytes() == img.tobytes()
    assert R.OPTIONAL == ((R.ACCUM_SECTION, 2), (R.ALT_SECTION, 3), (R.HYDROLOGY_SECTION, 4), (R.IRRIGATION_SECTION, 5))
    assert R.OPTIONAL_CELLS == ((7, 6), (8, 6)) and R.MAX_VERSION == 6


# ---- declarations ---------------------------------------------------------------------------------------------------------------------
def test_header_constants_and_bindings():
    import ctypes as C

    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert "enum { ELMK_CELL_ROWS_ROUTING = 0, ELMK_CELL_ROWS_SUPPLY = 1, ELMK_CELL_ROWS_NFAMILY = 2 };" in h
    assert "int elmk_cell_history_add_row(elmk_ctx *ctx, int tape, int family, int which, int op);" in h
    assert (st.CELL_ROWS_ROUTING, st.CELL_ROWS_SUPPLY) == (R.CELL_ROWS_ROUTING, R.CELL_ROWS_SUPPLY) == (0, 1)
    assert st.CELL_ROW_FAMILIES == {"routing": 0, "supply": 1}
    assert L.SIGNATURES["elmk_cell_history_add_row"] == (C.c_int, [C.c_void_p] + [C.c_int] * 4)
    assert hasattr(st.ELMState, "cell_history_add_row")
    assert "enum { ELMK_OPT_RESTART_CELLS = 3 };" in h and st.OPT_RESTART_CELLS == 3
    assert "enum { ELMK_RESTART_ROUTING = 7, ELMK_RESTART_IRRSUP = 8 };" in h and (R.ROUTING_SECTION, R.IRRSUP_SECTION) == (7, 8)
    assert "enum { ELMK_RESTART_VERSION_ROUTING = 6 };" in h and R.VERSION_ROUTING == 6
    assert re.search(r"Image format, version 6:", h)
    assert (hs.AVG, hs.SUM, hs.MAX, hs.MIN, hs.INST) == (st.HIST_AVG, st.HIST_SUM, st.HIST_MAX, st.HIST_MIN, st.HIST_INST) and hs.OPS == st.HIST_OPS
    hpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    assert "elmk_cell_history_add_row(" in hpp and "ELMK_OPT_RESTART_CELLS" in hpp
    if os.path.exists(L.LIB_PATH):
        import subprocess

        for path in (L.LIB_PATH, L.F32_LIB_PATH):
            syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
            assert re.search(r"\bT elmk_cell_history_add_row$", syms, re.M), path
