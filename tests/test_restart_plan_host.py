"""The chunk plan of restart images on the host (tests/restart_cases.py restates rst_plan of api_restart.cpp): the restatement's constants are
the source's, its section table is restart.build's, every size of test_gpu_restart_sizes.py has the property it was chosen for - so
that a change of a constant fails here instead of quietly emptying the GPU tests -, and RST_MAX_PIECES cannot be reached."""
import os
import re

import numpy as np

from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests import restart_cases as RC
from tests.support import ROOT

CSRC = os.path.join(ROOT, "elmkernels_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_are_the_sources():
    api = _src("api_restart.cpp")
    shift = re.search(r"constexpr size_t RST_CHUNK = \(size_t\)(\d+) << (\d+);", api)
    assert int(shift.group(1)) << int(shift.group(2)) == RC.CHUNK
    assert int(re.search(r"constexpr int RST_MAX_PIECES = (\d+);", api).group(1)) == RC.MAX_PIECES
    assert int(re.search(r"constexpr size_t RST_ALIGN = (\d+);", api).group(1)) == R.ALIGN
    nbx = re.search(r"P\.nbx\.push_back\(\(int\)std::min<int64_t>\((\d+), std::max<int64_t>\(1, \(maxn \+ (\d+)\) / (\d+)\)\)\);", api)
    assert (int(nbx.group(1)), int(nbx.group(2)) + 1, int(nbx.group(3))) == (RC.NBX_CAP, RC.BLOCK, RC.BLOCK)
    kern = _src("k_restart.hip")
    assert re.search(r"i = \(int64_t\)blockIdx\.x \* (\d+) \+ threadIdx\.x; i < P\.n; i \+= \(int64_t\)gridDim\.x \* (\d+)\)", kern).groups() == \
        (str(RC.THREADS),) * 2
    assert f"__launch_bounds__({RC.THREADS}) void k_rst_pieces" in kern


def test_layout_is_restart_builds():
    """The section table of restart_cases.layout against restart.build over zero-filled sections, with every kind of section."""
    n, cells = 70, 333
    sec, total = RC.layout(n, [(1, cells), (20, None)], [1, 20], RC.LARGE_OPTIONAL)
    data = [np.zeros((int(s["nlev"]), int(s["extent"])), R.ELEM[int(s["dtype"])]) for s in sec]
    h = np.zeros((), R.HEADER)
    h["magic"], h["ncols"] = R.MAGIC, n
    img = R.build(h, np.zeros(2, R.ENTRY), sec, data, np.zeros(2, R.ACCUM))
    p = R.parse(img)
    assert img.size == total and int(p["header"]["version"]) == R.VERSION_IRRIGATION
    assert p["sections"].tobytes() == sec.tobytes()
    assert sum(int(s["nlev"]) * R.ELEM[int(s["dtype"])].itemsize for s in sec if s["kind"] == R.FIELD) == 4053  # bytes per column


def test_with_section_is_a_rebuild():
    """restart_cases.with_section (an element changed under matching checksums, for the snl refusal at the large size) gives the bytes
    of restart.build, with and without the accumulator-count word and at a gcol0 beyond 32 bits."""
    for accum, optional in (([], ()), ([1], RC.LARGE_OPTIONAL)):
        sec, _ = RC.layout(37, [(1, None)], accum, optional)
        rng = np.random.default_rng(len(accum))
        data = [rng.integers(0, 200, (int(s["nlev"]), 37)).astype(R.ELEM[int(s["dtype"])]) for s in sec]
        h = np.zeros((), R.HEADER)
        h["magic"], h["ncols"], h["gcol0"] = R.MAGIC, 37, RC.LARGE_GCOL0
        for s, d in zip(sec, data):
            s["checksum"] = R.checksum(d, RC.LARGE_GCOL0)
        img = R.build(h, np.zeros(1, R.ENTRY), sec, data, np.zeros(len(accum), R.ACCUM))
        p = R.verify(img)
        i = 5
        data[i] = data[i].copy()
        data[i][-1, 3] += 1
        sec[i]["checksum"] = R.checksum(data[i], RC.LARGE_GCOL0)
        want = R.build(h, np.zeros(1, R.ENTRY), sec, data, np.zeros(len(accum), R.ACCUM))
        got = RC.with_section(img, p, i, data[i])
        assert got.tobytes() == want.tobytes() and got.tobytes() != img.tobytes()
        R.verify(got)


def _covers(sec, chunks):
    """Every element of every section lies in exactly one piece, at its image offset; chunks hold at most CHUNK bytes."""
    seen = {}
    for ch in chunks:
        assert 0 < ch.hi - ch.lo <= RC.CHUNK and ch.pieces[0].offset == 0
        for p in ch.pieces:
            S = sec[p.section]
            es = R.ELEM[int(S["dtype"])].itemsize
            assert ch.lo + p.offset == int(S["offset"]) + (p.level * int(S["extent"]) + p.first) * es
            assert ch.lo + p.offset + p.count * es <= ch.hi and p.count > 0
            assert seen.get((p.section, p.level), 0) == p.first  # the pieces of a row in order, without gaps
            seen[(p.section, p.level)] = p.first + p.count
    assert seen == {(s, lev): int(S["extent"]) for s, S in enumerate(sec) for lev in range(int(S["nlev"]))}


def test_gridded_sizes_reach_their_workgroup_counts():
    """GRID_CELLS: one chunk each; nbx and the trips of a workgroup over the widest piece are what the size was chosen for, and the
    70-element field rows run under the same nbx."""
    for ncells, (nbx, trips) in RC.GRID_CELLS.items():
        sec, total = RC.layout(RC.GRID_N, RC.grid_history(ncells))
        chunks = RC.plan(sec)
        _covers(sec, chunks)
        assert len(chunks) == 1 and total < RC.CHUNK, ncells
        widest = max(p.count for p in chunks[0].pieces)
        assert widest == ncells and min(p.count for p in chunks[0].pieces) == RC.GRID_N
        assert (chunks[0].nbx, RC.trips(widest, chunks[0].nbx)) == (nbx, trips), ncells
    sizes = sorted(RC.GRID_CELLS)
    assert sizes[0] == RC.BLOCK and sizes[1] == RC.BLOCK + 1  # either side of the second workgroup
    assert sizes[3] == RC.NBX_CAP * RC.BLOCK and sizes[4] == sizes[3] + 1  # either side of the first trip past BLOCK elements
    assert sizes[5] > 2 * sizes[3] and sizes[5] % (RC.NBX_CAP * RC.THREADS) not in (0, 1)  # beyond the next one, ragged


def test_gridded_cut_falls_inside_a_row_of_the_20_level_section():
    sec, _ = RC.layout(RC.GRID_N, RC.grid_history(RC.GRID_CUT_CELLS, levels20=True))
    chunks = RC.plan(sec)
    _covers(sec, chunks)
    assert len(chunks) == 2
    (cut,) = RC.cuts(chunks)
    S = sec[cut.section]
    assert (int(S["kind"]), int(S["nlev"]), int(S["extent"])) == (R.GRIDDED, 20, RC.GRID_CUT_CELLS)
    assert 0 < cut.first < RC.GRID_CUT_CELLS and cut.first + cut.count == RC.GRID_CUT_CELLS
    assert (RC.GRID_CUT_CELLS + 63) // 64 * 64 != RC.GRID_CUT_CELLS  # the accumulator's row stride is neither the extent nor ld
    assert cut.section < len(sec) - 1  # sections follow the cut row in the second chunk


def test_field_sizes_reach_their_workgroup_counts_and_cuts():
    for n, nbx in RC.FIELD_N_SMALL.items():
        sec, _ = RC.layout(n)
        chunks = RC.plan(sec)
        _covers(sec, chunks)
        assert len(chunks) == 1 and chunks[0].nbx == nbx and {p.count for p in chunks[0].pieces} == {n}, n
    assert 49000 <= RC.FIELD_N_LARGE <= 52000
    sec, total = RC.large_layout(RC.FIELD_N_LARGE)
    chunks = RC.plan(sec)
    _covers(sec, chunks)
    assert len(chunks) >= 4  # both staging slots reused: chunks 2 and 3 wait for the copies of chunks 0 and 1
    cut = RC.cuts(chunks)
    assert len(cut) == len(chunks) - 1 and all(0 < p.first < RC.FIELD_N_LARGE for p in cut)
    widths = [(int(sec[p.section]["kind"]), R.ELEM[int(sec[p.section]["dtype"])].itemsize) for p in cut]
    assert (R.FIELD, 8) in widths, "a cut inside a row of an F64 field"
    assert (R.FIELD, 4) in widths or (R.FIELD, 1) in widths, "a cut inside a row of a 4-byte or 1-byte field"
    assert any(p.level > 0 for p in cut)  # (the address of such a piece has both a level and a column term)
    # the history and the optional sections lie in the last chunk, and the last section of the last chunk is an irrigation row
    first_late = min(i for i, s in enumerate(sec) if s["kind"] != R.FIELD)
    assert all(p.section < first_late for ch in chunks[:-1] for p in ch.pieces)
    assert chunks[-1].pieces[-1].section == len(sec) - 1 and int(sec[-1]["kind"]) == R.IRRIGATION_SECTION
    assert all(ch.nbx == -(-RC.FIELD_N_LARGE // RC.BLOCK) for ch in chunks)
    assert RC.LARGE_GCOL0 + RC.FIELD_N_LARGE > 2**33 and total > 3 * RC.CHUNK


def test_the_piece_limit_cannot_be_reached():
    """A chunk holds at most every row of the image plus the one it begins inside.  The most rows a context can have: the image fields'
    levels, every history and accumulator entry over the widest field, and the optional rows - far below RST_MAX_PIECES."""
    hdr = open(os.path.join(ROOT, "include", "elmk.h")).read()
    hist = int(re.search(r"#define ELMK_HIST_MAX_ENTRIES (\d+)", hdr).group(1))
    accum = int(re.search(r"#define ELMK_ACCUM_MAX_ENTRIES (\d+)", hdr).group(1))
    assert (hist, accum) == (st.HIST_MAX_ENTRIES, st.ACCUM_MAX_ENTRIES)
    widest = max(nlev for _, nlev, _ in st.field_table().values())
    rows = sum(nlev for _, _, nlev, _ in RC.image_fields()) + (hist + accum) * widest + sum(RC.OPTIONAL_SECTIONS.values())
    assert len(RC.OPTIONAL_SECTIONS) + 1 == len(R.OPTIONAL)  # (every optional kind but the accumulators', counted above)
    assert rows + 1 < RC.MAX_PIECES, rows
    # and the plan of that context, at a size where everything is one chunk, has that many pieces
    sec, _ = RC.layout(RC.GRID_N, [(widest, None)] * hist, [widest] * accum, RC.LARGE_OPTIONAL)
    (chunk,) = RC.plan(sec)
    assert len(chunk.pieces) == rows
