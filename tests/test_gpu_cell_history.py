"""Cell rows on history tapes (include/elmk.h "cell rows on history tapes"): k_hist_accumulate_rows against the numpy fold
(elmkernels_amd/history.py) in both builds at the pair, workgroup and 64-cell boundaries and on a grid with far more cells than columns;
reset and read; the entries inside elmk_run against the stepwise calls, graph on and off, and an entry added between two runs; every
refusal and interlock, each leaving the context as it was; the tapes through a restart image beside the hand-carried rows; the routing
state in the image (ELMK_OPT_RESTART_CELLS, version 6): 3 + 3 = 6 with no _init call, the untouched images of the option off, every
refusal of a load."""
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import history as hs
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import cell_history_cases as cc
from tests import full_step_cases as fs
from tests.run_cases import schedule
from tests.support import bits, captured, same

pytestmark = pytest.mark.gpu

NSTEP = 5


def _assert_cell_tapes(D, ids, samples, what, rows=cc.CELL_ROWS):
    want = cc.host_results(samples, rows)
    n = len(samples)
    for (name, op), (entry, tape) in ids.items():
        got = D.history_read(entry)
        assert got.shape == want[(name, op)].shape, (what, name, op)
        assert (cc.canon(got) == cc.canon(want[(name, op)])).all(), (what, name, op, cc.differing(got, want[(name, op)]))
        if op == "avg":  # divided once, when read
            raw = hs.fold_cell_rows("avg", [s[name] for s in samples], raw=True)
            with np.errstate(all="ignore"):
                assert (cc.canon(got) == cc.canon(raw / np.float64(n))).all(), (what, name, "acc / count")


# ---- 1. the fold against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("ncells,ncols,with_columns", [(1, 130, None), (63, 166, None), (64, 168, None), (65, 170, None), (129, 298, None),
                                                       (513, 1066, None), (1001, 2042, None), (1001, 70, 20)])
def test_fold_equals_the_restatement(ncells, ncols, with_columns, lib_path):
    """Five chained steps (the irrigation with the limit, a prepared runoff row through the water balance, elmk_routing,
    elmk_history_accumulate) from storages with a NaN, an infinite, a negative and a 1e300 cell: all five ops over VOLR, QOUT, WF,
    FLOOD_FRAC and UNMET_SUM on two tapes against the numpy fold of the per-step reads, bit for bit with a NaN where the host has a NaN
    (cell_history_cases.canon says why), AVG = acc / count; a field entry, a column-row entry and two gridded entries on the same tapes
    against a second context that never added a cell-row entry; both counts 5.  The last case has 70 columns under 1001 cells: the
    launch's x extent is the cell rows', and 981 cells without a column are samples all the same."""
    G = cc.river_case(ncols, ncells, 300 + ncells + ncols, with_columns)
    if ncells >= 16:
        v = G["volr"]
        assert np.isnan(v).any() and np.isinf(v).any() and (v < 0).any() and (v == 1e300).any()
    A, B = cc.context(G, lib_path), cc.context(G, lib_path)
    bytes0 = A.device_bytes
    others_a, others_b = cc.add_other_entries(A), cc.add_other_entries(B)
    bytes1 = A.device_bytes
    ids = cc.add_cell_entries(A)
    cld = (ncells + 63) // 64 * 64
    assert A.device_bytes - bytes1 == len(ids) * 8 * cld and bytes1 - bytes0 == B.device_bytes - bytes0
    samples = []
    for k in range(NSTEP):
        cc.step(A, G, k)
        cc.step(B, G, k)
        samples.append(cc.read_cell_rows(A))
    assert any(bits(samples[0][n]) != bits(samples[-1][n]) for n in samples[0])
    if with_columns:
        empty = np.diff(G["map"][0]) == 0
        assert empty.sum() == ncells - with_columns and np.isfinite(samples[-1]["VOLR"][empty]).sum() > 900
    _assert_cell_tapes(A, ids, samples, (ncells, ncols))
    for (ea, ta), (eb, tb) in zip(others_a, others_b):
        assert ta == tb and same(A.history_read(ea), B.history_read(eb)), ("other entries", ea)
    assert A.history_count(0) == A.history_count(1) == B.history_count(0) == NSTEP
    for name in samples[0]:  # (the fold only reads its sources)
        assert bits(cc.read_cell_rows(A)[name]) == bits(cc.read_cell_rows(B)[name]), name
    A.close()
    B.close()


# ---- 2. reset and read ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def G70():
    return cc.river_case(193, 70, 410)


def test_reset_and_read(G70):
    """A reset of one tape leaves the other tape's cell accumulators and count alone and its own at the initial values (the next sample
    alone is what it then holds); a read at 0 samples and a read past ncells are refused; partial reads index cells."""
    G = G70
    D = cc.context(G)
    ids = cc.add_cell_entries(D)
    cc.add_other_entries(D)
    e_max, t_max = ids[("VOLR", "max")]
    with pytest.raises(L.ElmkError, match="no samples"):
        D.history_read(e_max)
    samples = []
    for k in range(3):
        cc.step(D, G, k)
        samples.append(cc.read_cell_rows(D))
    before = {key: D.history_read(e) for key, (e, t) in ids.items()}
    D.history_reset(0)
    assert D.history_count(0) == 0 and D.history_count(1) == 3
    for key, (e, t) in ids.items():
        if t == 1:
            assert bits(D.history_read(e)) == bits(before[key]), key
        else:
            with pytest.raises(L.ElmkError, match="no samples"):
                D.history_read(e)
    cc.step(D, G, 3)
    last = cc.read_cell_rows(D)
    for (name, op), (e, t) in ids.items():
        got = D.history_read(e)
        want = hs.fold_cell_rows(op, [last[name]] if t == 0 else [s[name] for s in samples] + [last[name]])
        assert (cc.canon(got) == cc.canon(want)).all(), (name, op, t)
    e, _ = ids[("QOUT", "sum")]
    full = D.history_read(e)
    assert bits(D.history_read(e, col0=33, n=37)) == bits(full[33:]) and D.history_read(e, col0=69, n=1).shape == (1,)
    assert bits(D.history_read(e, layout=77)) == bits(full)  # one level: the layout is not looked at
    for col0, n in ((0, 71), (70, 1), (64, 7), (-1, 2)):
        with pytest.raises(L.ElmkError, match="range"):
            D.history_read(e, col0=col0, n=n)
    D.close()


def test_avg_tape_of_qout_is_the_routing_mean(G70):
    """An AVG tape of QOUT reset together with elmk_routing_reset_mean equals QOUT_SUM / ncalls under ==, over finite storages."""
    G = dict(G70)
    for k in ("volr", "wh", "wt", "wf"):
        G[k] = cc.finite(G[k])
    for kinematic in (True, False):
        D = cc.context(G, kinematic=kinematic, supply=False)
        e = D.cell_history_add_row(2, "routing", rt.QOUT, "avg")
        for k in range(2):
            cc.step(D, G, k)
        D.history_reset(2)
        D.routing_reset_mean()
        for k in range(2, 6):
            cc.step(D, G, k)
        assert D.routing_count() == D.history_count(2) == 4
        mean = D.routing_read(rt.QOUT_SUM) / 4.0
        got = D.history_read(e)
        assert np.isfinite(mean).all() and mean.any() and (got == mean).all(), kinematic
        D.close()


# ---- 3. the run ----------------------------------------------------------------------------------------------------------------------
def _full(graph, **kw):
    D = fs.full_context(graph, **kw)
    D._cell = cc.add_cell_entries(D)
    D._hist += list(D._cell.values())
    return D


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(graph):
    """Six steps of elmk_run with every stage on against the stand-alone calls in the step's order, on every entry and everything else a
    step changes; then an entry added between two runs on a tape of its own samples the second run's six steps (the captured step is
    re-captured through hist_version), again as the stepwise calls do."""
    G = fs.case()
    S = schedule(fs.NSTEPS)
    A, B = _full(False), _full(graph)
    fs.full_stepwise(A, G["rec"], S[:6])
    fs.run(B, S[:6])
    B.sync()
    want, got = fs.full_snapshot(A), fs.full_snapshot(B)
    diag = [k for k in want if k.startswith("diag/")]
    fs.assert_same_snapshot(got, want, "six steps", skip=diag)
    assert all(got[f"hist/{e}"][0] == 6 for e, _ in B._cell.values())
    for D in (A, B):
        D._late = D.cell_history_add_row(2, "routing", rt.FLOOD_DEPTH, "max")
        D._hist.append((D._late, 2))
    fs.full_stepwise(A, G["rec"], S[6:])
    fs.run(B, S[6:])
    B.sync()
    want, got = fs.full_snapshot(A), fs.full_snapshot(B)
    fs.assert_same_snapshot(got, want, "twelve steps", skip=diag)
    assert B.history_count(2) == 6 and B.history_count(0) == 12 and got[f"hist/{B._late}"][1].any()
    A.close()
    B.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def _everything(D, ids):
    out = {f"route/{w}": D.routing_read(w) for w in range(10)}
    out.update({f"sup/{w}": D.irrigation_supply_read(w) for w in range(4)})
    for key, (e, t) in ids.items():
        out[f"hist/{key}"] = D.history_read(e)
    out["bytes"] = np.array(D.device_bytes)
    out["counts"] = np.array([D.history_count(t) for t in range(st.HIST_MAX_TAPES)])
    return out


def _assert_untouched(D, ids, before, what):
    now = _everything(D, ids)
    differ = [k for k in before if not same(now[k], before[k])]
    assert not differ, (what, differ)


def test_refusals_change_nothing(G70):
    G = G70
    D = cc.context(G)
    ids = cc.add_cell_entries(D, rows=cc.CELL_ROWS[:3], ops=("avg", "max"))
    for k in range(2):
        cc.step(D, G, k)
    before = _everything(D, ids)
    add = D.cell_history_add_row
    refused = [("unknown cell-row family", lambda: add(2, 2, 0, "avg")), ("unknown cell-row family", lambda: add(2, -1, 0, "avg")),
               ("row out of range", lambda: add(2, "routing", 10, "avg")), ("row out of range", lambda: add(2, "routing", -1, "avg")),
               ("row out of range", lambda: add(2, "supply", 4, "avg")), ("unknown op", lambda: add(2, "routing", rt.VOLR, 5)),
               ("unknown tape", lambda: add(4, "routing", rt.VOLR, "avg")), ("holds samples", lambda: add(0, "routing", rt.VOLR, "avg"))]
    for text, call in refused:
        with pytest.raises(L.ElmkError, match=text):
            call()
        _assert_untouched(D, ids, before, text)
    with captured(D):
        with pytest.raises(L.ElmkError, match="captured"):
            add(2, "routing", rt.VOLR, "avg")
    _assert_untouched(D, ids, before, "capture")
    # the interlocks: refused while an entry exists on the rows the call would free
    for text, call in (("elmk_routing_clear", D.routing_clear), ("elmk_routing_inundation_clear", D.routing_inundation_clear),
                       ("elmk_routing_kinematic_clear", D.routing_kinematic_clear), ("elmk_clear_output_grid", D.clear_output_grid),
                       ("elmk_set_output_grid", lambda: D.set_output_grid(*G["map"], fill=0.0))):
        with pytest.raises(L.ElmkError, match=text + ".*elmk_history_clear first|" + text + ".*clear first"):
            call()
        _assert_untouched(D, ids, before, text)
    D.close()


def test_interlocks_name_the_entries_and_end_with_the_clear(G70):
    """Each interlocked call alone against an entry on the rows it would free: refused with "cell-row history entries", everything as it
    was, and accepted after elmk_history_clear."""
    G = G70
    cases = (("supply", ir.UNMET_SUM, "irrigation_supply_clear", {}), ("routing", rt.WF, "routing_inundation_clear", {}),
             ("routing", rt.WT, "routing_kinematic_clear", dict(flood=False, supply=False)),
             ("routing", rt.QOUT, "routing_clear", dict(supply=False)))
    for fam, which, clear, kw in cases:
        D = cc.context(G, **kw)
        e = D.cell_history_add_row(0, fam, which, "max")
        cc.step(D, G, 0)
        ids = {"e": (e, 0)}
        rows = {w: D.routing_read(w) for w in range(4)}
        got, nbytes = D.history_read(e), D.device_bytes
        with pytest.raises(L.ElmkError, match="elmk_" + clear + ": cell-row history entries.*elmk_history_clear first"):
            getattr(D, clear)()
        assert same(D.history_read(e), got) and D.device_bytes == nbytes and all(same(D.routing_read(w), rows[w]) for w in rows), clear
        D.history_clear()
        getattr(D, clear)()
        assert D.device_bytes < nbytes
        D.close()
        del ids
    # the grid calls: the routing's own interlock stands in front of them while it is enabled, so theirs shows against a context whose
    # entries outlive nothing else - checked through the message of the first refusal that applies
    D = cc.context(G, supply=False)
    D.cell_history_add_row(1, "routing", rt.VOLR, "inst")
    for call in (D.clear_output_grid, lambda: D.set_output_grid(*G["map"], fill=0.0)):
        with pytest.raises(L.ElmkError, match="cell-row history entries.*elmk_history_clear first"):
            call()
    D.history_clear()
    D.routing_clear()
    D.clear_output_grid()
    D.close()


def test_rows_follow_what_is_enabled(G70):
    """The routing family takes exactly the rows elmk_routing_read takes at the moment of the call; the supply family needs the limit."""
    G = G70
    D = cc.context(G, routing=False)
    with pytest.raises(L.ElmkError, match="runoff routing is not enabled .elmk_routing_enable"):
        D.cell_history_add_row(0, "routing", rt.VOLR, "avg")
    with pytest.raises(L.ElmkError, match="supply limit is not on .elmk_irrigation_supply_enable"):
        D.cell_history_add_row(0, "supply", ir.UNMET_SUM, "avg")
    nbytes = D.device_bytes
    cc.enable_routing(D, G, kinematic=False, supply=False)
    for w in (rt.WH, rt.WT, rt.QSUR):
        with pytest.raises(L.ElmkError, match="kinematic-wave scheme is not on .elmk_routing_kinematic_enable"):
            D.cell_history_add_row(0, "routing", w, "avg")
    D.routing_kinematic_enable(G["params"])
    for w in (rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC):
        with pytest.raises(L.ElmkError, match="floodplain inundation is not on .elmk_routing_inundation_enable"):
            D.cell_history_add_row(0, "routing", w, "avg")
    e = [D.cell_history_add_row(0, "routing", w, "inst") for w in (rt.QIN, rt.QOUT_SUM, rt.WH, rt.QSUR)]
    D.routing_init(cc.finite(G["volr"]))
    cc.step(D, G, 0)
    for entry, w in zip(e, (rt.QIN, rt.QOUT_SUM, rt.WH, rt.QSUR)):
        assert bits(D.history_read(entry)) == bits(D.routing_read(w)), w
    D.history_clear()
    D.routing_clear()
    assert D.device_bytes == nbytes
    D.close()


# ---- 5. the tapes through a restart image ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_cell_tapes_restart_3_plus_3(lib_path):
    """Three steps, an image, a fresh context with the same stages and entries, the river stages' prognostic rows handed over through
    their read / init pairs, three more steps: every tape, cell-row tapes included (saved mid-interval with 3 samples), and everything
    else a step changes equal the six-step run bit for bit.  The image's entry table names the cell-row entries (gridded = 2, the
    routing's ncells, ELMK_RESTART_ROW_FIELD(ELMK_ROWS_NFAMILY + family, which)); restart.merge and restart.slice refuse it; a context
    without the entries refuses it with everything untouched."""
    S = schedule(fs.NSTEPS)
    A = _full(True, lib_path=lib_path)
    fs.run(A, S[:6])
    want = fs.full_snapshot(A)
    A.close()
    B = _full(True, lib_path=lib_path)
    fs.run(B, S[:3])
    img = B.restart_save()
    carried = dict(route=[B.routing_read(w) for w in (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF)], count=B.routing_count(),
                   unmet=B.irrigation_supply_read(ir.UNMET_SUM), alt=[B.active_layer_read(w) for w in range(3)])
    p = R.verify(img)
    ent = p["entries"]
    cell = ent[ent["gridded"] == 2]
    assert len(cell) == len(B._cell) and (cell["ncells"] == fs.NCELL).all()
    assert R.entry_row(cell["field"][0]) == (st.ROWS_IRRIGATION + 1 + st.CELL_ROWS_ROUTING, rt.VOLR)
    assert R.entry_row(cell["field"][-1]) == (st.ROWS_IRRIGATION + 1 + st.CELL_ROWS_SUPPLY, ir.UNMET_SUM)
    secs = p["sections"]
    assert (secs["extent"][(secs["kind"] == R.GRIDDED)] == fs.NCELL).all()
    for call in (lambda: R.merge([img]), lambda: R.slice(img, 0, 10)):
        with pytest.raises(R.RestartError, match="gridded|cell-row"):
            call()
    B.close()
    N = fs.full_context(True, lib_path=lib_path, init=False)  # the same stages, the older entries only
    before = fs.full_snapshot(N)
    with pytest.raises(L.ElmkError, match="history entries"):
        N.restart_load(img)
    fs.assert_same_snapshot(fs.full_snapshot(N), before, "refused load")
    N.close()
    C = _full(True, lib_path=lib_path, init=False, poisoned=True)
    C.restart_load(img)
    volr, qsum, wh, wt, wf = carried["route"]
    C.routing_init(volr, qsum, carried["count"])
    C.routing_kinematic_init(wh, wt)
    C.routing_inundation_init(wf)
    C.irrigation_supply_init(carried["unmet"])
    assert all(C.history_count(t) == 3 for t in (0, 1))
    fs.run(C, S[3:6])
    got = fs.full_snapshot(C)
    fs.assert_same_snapshot(got, want, "3 + 3", skip=[k for k in want if k.startswith("diag/")])
    C.close()


# ---- 6. the routing state in the image (ELMK_OPT_RESTART_CELLS, version 6) -------------------------------------------------------------
def _ers(lib_path, linear):
    """3 + 3 = 6 through a version-6 image with no _read / _init pair; linear: the linear scheme alone, without the limit."""
    S = schedule(fs.NSTEPS)

    def make(init, poisoned=False):
        kw = dict(lib_path=lib_path, init=init, poisoned=poisoned)
        if linear:
            D = fs.full_context(True, thr=None, **kw)
            D.routing_inundation_clear()
            D.routing_kinematic_clear()
            if init:
                D.routing_init(fs.case()["volr"])
            D._cell = cc.add_cell_entries(D, rows=cc.LINEAR_ROWS)
            D._hist += list(D._cell.values())
        else:
            D = _full(True, **kw)
        D.set_option(st.OPT_RESTART_CELLS, 1)
        return D

    A = make(True)
    fs.run(A, S[:6])
    want = fs.full_snapshot(A)
    A.close()
    B = make(True)
    fs.run(B, S[:3])
    assert B.restart_size() == B.restart_save().size
    img = B.restart_save()
    B.close()
    p = R.verify(img)
    assert int(p["header"]["version"]) == R.VERSION_ROUTING == 6 and p["routing_ncalls"] == 3
    ids = [int(s["id"]) for s in p["sections"] if int(s["kind"]) == R.ROUTING_SECTION]
    assert ids == ([rt.VOLR, rt.QOUT_SUM] if linear else [rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF])
    sup = [int(s["id"]) for s in p["sections"] if int(s["kind"]) == R.IRRSUP_SECTION]
    assert sup == ([] if linear else [ir.UNMET_SUM])
    tail = p["sections"][-(len(ids) + len(sup)):]
    assert (tail["extent"] == fs.NCELL).all() and (tail["nlev"] == 1).all() and set(tail["kind"]) <= {R.ROUTING_SECTION, R.IRRSUP_SECTION}
    for call in (lambda: R.merge([img]), lambda: R.slice(img, 0, 10)):
        with pytest.raises(R.RestartError):
            call()
    C = make(False, poisoned=True)
    C.restart_load(img)
    assert C.routing_count() == 3 and not C.routing_read(rt.QIN).any() and not C.routing_read(rt.QOUT).any()
    if not linear:
        assert not any(C.routing_read(w).any() for w in (rt.QSUR, rt.FLOOD_DEPTH, rt.FLOOD_FRAC))
        assert not any(C.irrigation_supply_read(w).any() for w in (ir.DEMAND, ir.COMMITTED, ir.RATIO))
    fs.run(C, S[3:6])
    fs.assert_same_snapshot(fs.full_snapshot(C), want, "3 + 3 through version 6", skip=[k for k in want if k.startswith("diag/")])
    C.close()


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_version_6_restart_3_plus_3(lib_path):
    """Every stage on, every row of the river stages, the call count and every tape, cell-row tapes included, saved mid-interval with 3
    samples: the bits of the six-step run, with no _read / _init pair."""
    _ers(lib_path, linear=False)


def test_version_6_restart_with_the_linear_scheme():
    _ers(None, linear=True)


def test_option_off_changes_no_image():
    """With the option off, or switched on and off again, and no cell-row entries: the size and the bytes of a context that never
    touched it, routing enabled or not."""
    S = schedule(fs.NSTEPS)
    imgs = []
    for touch in (False, True):
        D = fs.full_context(True)
        if touch:
            D.set_option(st.OPT_RESTART_CELLS, 1)
            assert D.restart_size() > imgs[0].size
            D.set_option(st.OPT_RESTART_CELLS, 0)
        fs.run(D, S[:2])
        assert D.restart_size() == D.restart_save().size
        imgs.append(D.restart_save())
        if touch:  # without the routing the option changes nothing
            D.set_option(st.OPT_RESTART_CELLS, 1)
            D.irrigation_supply_clear()
            D.routing_clear()
            assert D.restart_size() == imgs[0].size and int(R.parse(D.restart_save())["header"]["version"]) == R.VERSION_IRRIGATION
        D.close()
    assert bits(imgs[0]) == bits(imgs[1]) and int(R.parse(imgs[0])["header"]["version"]) == R.VERSION_IRRIGATION


def test_version_6_load_refusals():
    """Each refused with everything untouched and the context usable: a version-6 image into a context without the routing, with
    another ncells, with the kinematic-wave scheme off, with the option off; a version-5 image into a context with the option on and
    the routing enabled; a version-6 image with one flipped byte in the VOLR section; the option under a captured stream."""
    G = cc.river_case(193, 70, 410)
    S6 = cc.context(G)
    S6.set_option(st.OPT_RESTART_CELLS, 1)
    cc.step(S6, G, 0, sample=False)
    img6 = S6.restart_save()
    p = R.verify(img6)
    assert int(p["header"]["version"]) == 6 and p["routing_ncalls"] == 1
    S6.set_option(st.OPT_RESTART_CELLS, 0)
    img5 = S6.restart_save()
    assert int(R.verify(img5)["header"]["version"]) == R.VERSION_IRRIGATION and img5.size < img6.size
    volr = next(i for i, s in enumerate(p["sections"]) if int(s["kind"]) == R.ROUTING_SECTION and int(s["id"]) == rt.VOLR)
    flipped = img6.copy()
    flipped[int(p["sections"][volr]["offset"]) + 8 * 20 + 3] ^= 0x10
    with pytest.raises(R.RestartError, match="checksum"):
        R.verify(flipped)
    S6.close()
    G65 = cc.river_case(193, 65, 411)

    def target(what):
        if what == "other ncells":
            D = cc.context(G65)
        else:
            D = cc.context(G, routing=what != "no routing", kinematic=what != "kinematic off")
        D.set_option(st.OPT_RESTART_CELLS, what != "option off")
        return D

    cases = (("no routing", img6, "routing state.*not enabled.*elmk_routing_enable"),
             ("other ncells", img6, "routing state differs.*ncells .elmk_routing_enable"),
             ("kinematic off", img6, "routing state differs.*elmk_routing_kinematic_enable"),
             ("option off", img6, "routing state.*not enabled.*ELMK_OPT_RESTART_CELLS"),
             ("version 5", img5, "context has the routing state.*version-5 image holds no such rows"),
             ("flipped", flipped, "section checksum mismatch"))
    for what, img, text in cases:
        D = target(what)
        GG = G65 if what == "other ncells" else G
        if what != "no routing":
            cc.step(D, GG, 1, sample=False)
        fields ={k: D[k] for k in D.fields}
        rows = [D.routing_read(w) for w in range(4)] if what != "no routing" else []
        count = D.routing_count() if what != "no routing" else None
        with pytest.raises(L.ElmkError, match=text):
            D.restart_load(img)
        assert all(same(D[k], fields[k]) for k in fields), what
        if what != "no routing":
            assert all(same(D.routing_read(w), rows[w]) for w in range(4)) and D.routing_count() == count, what
            cc.step(D, GG, 2, sample=False)  # usable
            assert D.routing_count() == count + 1
        D.close()
    D = target("loads")
    D.restart_load(img6)
    assert D.routing_count() == 1
    with captured(D):
        with pytest.raises(L.ElmkError, match="captured"):
            D.set_option(st.OPT_RESTART_CELLS, 0)
    D.close()


# ---- 7. the example ---------------------------------------------------------------------------------------------------------------------
def test_river_output_demo_runs(tmp_path):
    from tests.support import build_demo, run_demo

    r = run_demo(build_demo("river_output_demo", tmp_path))
    assert "identical" in r.stdout and "DIFFERENT" not in r.stdout and "version-6 image" in r.stdout, r.stdout
    rows = [ln.split() for ln in r.stdout.splitlines() if re.match(r"\s+\d+\s", ln)]
    assert len(rows) == 8 and float(rows[-1][2]) > float(rows[-1][1]) > 0.0  # the outlet's peak above its mean
