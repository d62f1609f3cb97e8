"""Restart images past one workgroup per row and past one staging chunk (k_restart.hip, api_restart.cpp), at the sizes of
tests/restart_cases.py, whose properties tests/test_restart_plan_host.py asserts: rows of 4096 .. 524 588 elements in a 70-column
context through wide gridded history sections, a chunk boundary inside a 20-level gridded section, field rows under 2 and 3
workgroups, and a four-chunk image with cuts inside F64 and 4-byte field rows in both builds, saved at a global column past 2^33.
The references are elmk_download, the features' own reads and restart.py's numpy checksums.

nbx, the workgroups per row, is taken from the widest piece of a chunk, so in the gridded cases the 70-element field rows run with
up to 64 workgroups of which 63 see no element; their zero partials are summed into every field section's checksum, which
restart.verify recomputes in its own order."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as HY
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests import restart_cases as RC
from tests.support import same

pytestmark = pytest.mark.gpu


# ---- rows past one workgroup, at 70 columns ---------------------------------------------------------------------------------------------
def _grid_context(ncells, entries, poisoned):
    """70 columns under a map of ncells cells - cell k averages column k % 70 with weight 1 + k 2^-20, so no two cells accumulate the
    same bits -, the gridded entries and one column entry on tape 0; accumulated twice with t_grnd and t_soisno changed in between
    (poisoned: every field filled with NaN or 3 and accumulated once)."""
    n = RC.GRID_N
    D = st.ELMState(n)
    k = np.arange(ncells)
    D.set_output_grid(np.arange(ncells + 1, dtype=np.int64), (k % n).astype(np.int32), 1.0 + k * 2.0**-20, -1.0)
    ids = [D.gridded_history_add(0, name, op) for name, op in entries] + [D.history_add(0, "h2osno", "sum")]
    if poisoned:
        RC.poison_fields(D)
        D.history_accumulate()
        return D, ids
    RC.fill_pattern(D, only_image=True)
    for step in range(2):  # finite sources: an average is section / count, bit for bit, only without NaN payloads
        D["t_grnd"] = 250.0 + RC.column_rows(n, 0, step)
        D["t_soisno"] = 240.0 + np.stack([RC.column_rows(n, lev, step) for lev in range(D.fields["t_soisno"][1])], axis=1)
        D["h2osno"] = RC.column_rows(n, 30, step)
        D.history_accumulate()
    return D, ids


def _reads(D, ids):
    return [D.history_read(e, layout=st.LAYOUT_SOA) for e in ids], [D.history_count(t) for t in range(st.HIST_MAX_TAPES)]


def _grid_case(ncells, entries):
    A, ids = _grid_context(ncells, entries, False)
    img = A.restart_save()
    assert img.size == A.restart_size()
    p = R.verify(img)  # restart.py's checksums of every section against the device's
    want, counts = _reads(A, ids)
    assert counts == [2, 0, 0, 0]
    nsec = 0
    for s, d in zip(p["sections"], p["data"]):
        if int(s["kind"]) == R.GRIDDED:
            e = int(s["id"])
            assert d.shape[1] == ncells
            got = d / 2.0 if entries[e][1] == "avg" else d  # the raw accumulator; history_read divides an average by the count
            assert same(got.reshape(want[e].shape), want[e]), (ncells, e)
            nsec += 1
    assert nsec == len(entries)
    B, ids_b = _grid_context(ncells, entries, True)
    B.restart_load(img)
    got, counts_b = _reads(B, ids_b)
    assert counts_b == counts
    for e, (x, y) in enumerate(zip(got, want)):
        assert same(x, y), (ncells, e)
    # one more sample in both: every field, accumulator and count stays equal (the images hold them all; a read of a wide gridded
    # entry goes through the small staging buffer of a 70-column context, many round trips each)
    A.history_accumulate()
    B.history_accumulate()
    again = B.restart_save()
    assert same(again, A.restart_save()) and not same(again, img)
    assert B.history_count(0) == 3
    A.close()
    B.close()


@pytest.mark.parametrize("ncells", list(RC.GRID_CELLS))
def test_gridded_rows_past_one_workgroup(ncells):
    """Gridded sections of ncells elements with every reducing op: the image verifies, each section is its entry's history_read, and a
    poisoned context that loads it reads the same, before and after one more accumulate on both."""
    _grid_case(ncells, RC.GRID_ENTRIES)


def test_chunk_boundary_inside_a_gridded_section():
    """A 20-level gridded section of more than one chunk: the second piece of the cut row starts at a cell offset of an accumulator
    whose row stride is its own, not the state's."""
    _grid_case(RC.GRID_CUT_CELLS, RC.GRID_ENTRIES_CUT)


# ---- field rows past one workgroup and past one chunk ---------------------------------------------------------------------------------------
def _field_context(n, lib_path, poisoned):
    """Every field by upload from restart_cases.pattern, an accumulator entry, the active layer, the soil hydrology and the irrigation with
    per-column distinct rows (the row alt is only ever zero without a run), two column history entries sampled twice.  poisoned: every
    field filled with NaN or 3, other rows and step counts, one sample."""
    D = st.ELMState(n, lib_path=lib_path)
    acc = D.accum_add("t_grnd", "runmean", 10)
    D.active_layer_enable()
    D.soil_hydrology_enable()
    D.irrigation_enable((np.arange(n) * 7919 % 86401 - 1).astype(np.int32))
    ids = [D.history_add(1, name, op) for name, op in RC.LARGE_HISTORY]
    s = 1 if poisoned else 0
    if poisoned:
        RC.poison_fields(D)
    else:
        RC.fill_pattern(D)
    D.accum_init(acc, RC.column_rows(n, 1, s), nsteps=7 + 5 * s)
    D.active_layer_init(RC.column_rows(n, 2, s), RC.column_rows(n, 3, s))
    D.soil_hydrology_init(RC.column_rows(n, 4, s), 4000.0 + RC.column_rows(n, 5, s))
    D.irrigation_init(RC.column_rows(n, 6, s), ((np.arange(n) * 31 + 17 * s) % 86401).astype(np.float64))  # NLEFT: whole seconds
    D.history_accumulate()
    if not poisoned:
        fid, nlev, dt = D.fields["t_grnd"]
        D["t_grnd"] = RC.pattern("t_grnd", fid, nlev, dt, n, salt=2)
        D.history_accumulate()
    return D, acc, ids


def _rows(D, acc, ids):
    """Everything of the context outside its fields that an image holds, as the features' own reads give it."""
    val, nsteps = D.accum_read(acc)
    out = {("accum", 0): val, "accum steps": nsteps, "tape counts": [D.history_count(t) for t in range(st.HIST_MAX_TAPES)]}
    for w in range(3):
        out[("alt", w)] = D.active_layer_read(w)
    for w in (HY.ZWT, HY.WA):
        out[("hyd", w)] = D.soil_hydrology_read(w)
    for w in range(st.IRR_NROWS):
        out[("irr", w)] = D.irrigation_read(w)
    for e in ids:
        out[("hist", e)] = D.history_read(e, layout=st.LAYOUT_SOA)
    return out


def _assert_same_rows(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert same(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


SECTION_ROWS = {R.ACCUM_SECTION: "accum", R.ALT_SECTION: "alt", R.HYDROLOGY_SECTION: "hyd", R.IRRIGATION_SECTION: "irr", R.HISTORY: "hist"}


def _assert_image(D, img, p, gcol0, fields, rows):
    """(a) the size, and restart.py's checksums at gcol0 against the device's (p = restart.parse(img)); (b) every field section is
    elmk_download, every other section its feature's read.  In an image of one chunk every section is summed in numpy; in a larger
    one the sections a chunk boundary cuts, the first of each element type and every section after the fields - the others are
    compared with the downloads alone, and their sums by the load, on the device."""
    assert img.size == D.restart_size()
    h, sec = p["header"], p["sections"]
    assert R.header_checksum(img, int(h["header_bytes"])) == int(h["header_checksum"])
    chunks = RC.plan(sec)
    summed = set(range(len(sec)))
    if len(chunks) > 1:
        first = {int(s["dtype"]): i for i, s in reversed(list(enumerate(sec)))}
        summed = {c.section for c in RC.cuts(chunks)} | set(first.values()) | {i for i, s in enumerate(sec) if int(s["kind"]) != R.FIELD}
        assert len(first) == len(R.ELEM) and len(RC.cuts(chunks)) == len(chunks) - 1
    for i in sorted(summed):
        assert R.checksum(p["data"][i], gcol0) == int(sec[i]["checksum"]), (int(sec[i]["kind"]), int(sec[i]["id"]))
    assert int(h["gcol0"]) == gcol0 and int(h["version"]) == R.VERSION_IRRIGATION
    by_id = {fid: name for name, (fid, _, _) in D.fields.items()}
    seen = []
    for s, d in zip(p["sections"], p["data"]):
        kind, sid = int(s["kind"]), int(s["id"])
        if kind == R.FIELD:
            want = fields[by_id[sid]]
            assert same(d, np.ascontiguousarray(want.reshape(D.ncols, -1).T)), by_id[sid]
        else:
            assert same(d.reshape(rows[(SECTION_ROWS[kind], sid)].shape), rows[(SECTION_ROWS[kind], sid)]), (kind, sid)
        seen.append((kind, sid))
    want_fields = [(R.FIELD, fid) for _, fid, _, _ in RC.image_fields()]
    assert seen == want_fields + [(R.HISTORY, 0), (R.HISTORY, 1), (R.ACCUM_SECTION, 0)] + [(R.ALT_SECTION, w) for w in range(3)] + \
        [(R.HYDROLOGY_SECTION, w) for w in range(2)] + [(R.IRRIGATION_SECTION, w) for w in range(2)]


class Saved:
    """A context of n columns saved at gcol0, with what the image is compared against; one per (n, build), shared by its tests."""

    def __init__(self, n, lib_path, gcol0):
        self.n, self.lib_path, self.gcol0 = n, lib_path, gcol0
        self.D, self.acc, self.ids = _field_context(n, lib_path, False)
        self.fields = RC.fields_of(self.D)
        self.rows = _rows(self.D, self.acc, self.ids)
        self.img = self.D.restart_save(gcol0)
        self.parsed = R.parse(self.img)

    def poisoned(self):
        return _field_context(self.n, self.lib_path, True)


def _round_trip(S):
    """(a), (b); (c) a poisoned context loads the image and equals the saved one in every image field, row, accumulator, count and tape
    count, its other fields as poisoned as they were; (d) its own save is the image byte for byte."""
    _assert_image(S.D, S.img, S.parsed, S.gcol0, S.fields, S.rows)
    P, acc, ids = S.poisoned()
    before = RC.fields_of(P)
    P.restart_load(S.img, S.gcol0)
    after = RC.fields_of(P)
    image = {k for k in after if st.field_class(k) in RC.IMAGE_CLASSES}
    RC.assert_same_fields({k: S.fields[k] for k in image}, {k: after[k] for k in image}, "loaded")
    RC.assert_same_fields({k: v for k, v in before.items() if k not in image}, {k: v for k, v in after.items() if k not in image}, "outside the image")
    _assert_same_rows(S.rows, _rows(P, acc, ids), "loaded")
    assert same(P.restart_save(S.gcol0), S.img)
    P.close()


@pytest.mark.parametrize("n,lib_path", [(4097, None), (4097, L.F32_LIB_PATH), (8193, None)], ids=["4097-f64", "4097-f32", "8193-f64"])
def test_field_rows_past_one_workgroup(n, lib_path):
    S = Saved(n, lib_path, 12345)
    _round_trip(S)
    S.D.close()


@pytest.fixture(scope="module", params=[None, L.F32_LIB_PATH], ids=["f64", "f32"])
def large(request):
    S = Saved(RC.FIELD_N_LARGE, request.param, RC.LARGE_GCOL0)
    yield S
    S.D.close()


def test_four_chunks_round_trip(large):
    """FIELD_N_LARGE columns: four chunks through both staging slots, cuts inside F64 and 4-byte field rows (in the fp32-state build
    the stored element of a cut F64 row is 4 bytes against the image's 8), the history and optional sections in the last chunk, and a
    checksum origin beyond 32 bits."""
    _round_trip(large)


def test_a_refused_load_leaves_the_first_chunks_alone(large):
    """The load verifies every chunk before it scatters any: an image whose last section of the last chunk has one bit flipped, and one
    with an snl of 6 under a matching checksum, are refused with every field and row of the poisoned context as it was, the fields of
    the first chunk included."""
    S = large
    p = S.parsed
    last = p["sections"][-1]
    flipped = S.img.copy()
    flipped[int(last["offset"]) + 8 * (S.n - 1) + 3] ^= 0x04
    i = [int(s["kind"]) == R.FIELD and int(s["id"]) == S.D.fields["snl"][0] for s in p["sections"]].index(True)
    snl = p["data"][i].copy()
    snl[0, S.n - 2] = 6
    bad_snl = RC.with_section(S.img, p, i, snl)
    P, acc, ids = S.poisoned()
    fields, rows = RC.fields_of(P), _rows(P, acc, ids)
    for what, bad in (("section checksum mismatch", flipped), ("snl outside", bad_snl)):  # (the patched checksums pass: snl is the reason)
        with pytest.raises(L.ElmkError, match=what):
            P.restart_load(bad, S.gcol0)
        RC.assert_same_fields(fields, RC.fields_of(P), what)
        _assert_same_rows(rows, _rows(P, acc, ids), what)
    P.restart_load(S.img, S.gcol0)  # and the context still loads the image itself
    _assert_same_rows(S.rows, _rows(P, acc, ids), "after the refusals")
    P.close()
