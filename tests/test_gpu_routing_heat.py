"""Stream temperature on the device (include/elmk.h "stream temperature"): the HEAT form of k_kinematic_prep and k_kinematic_step
against the host restatement (routing.kinematic_call(heat=...)) bit for bit on the seven new rows and the seven water rows, in both
builds, over five chained calls on every network shape, size and nsub, the withdrawal on and off, with the edge values in cells of
their own; the stage inside elmk_run against the stepwise calls, graph on and off; restarts through _read and _init and through a
version-8 image; a row on a history tape; the clear; every refusal and interlock; the budget; the example."""
import ctypes as C
import functools

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import history as hs
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import heat_cases as hc
from tests import river_cases as rv
from tests.hydrology_cases import _new
from tests.river_cases import NCELL, NCOL, NSTEPS, TOL, differing, finite, host_inputs, read_rows, river_snapshot, set_runoff
from tests.run_cases import DT, NREC, assert_same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

KW_ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR)
HEAT_ROWS = (rt.TT, rt.TR, rt.HEAT, rt.HIN, rt.HSRF, rt.HADJ, rt.HOUT)
ROWS = KW_ROWS + HEAT_ROWS
NAMES = dict(zip(ROWS, ("VOLR", "QIN", "QOUT", "QOUT_SUM", "WH", "WT", "QSUR", "TT", "TR", "HEAT", "HIN", "HSRF", "HADJ", "HOUT")))
NAN, INF = hc.NAN, hc.INF


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return rv.base()


def set_columns(D, call, ncols=hc.NCOLS):
    """The column fields of H1 onto the device; returns them as the device stores them (the fp32-state build rounds)."""
    for k, v in hc.columns(ncols, 77, call).items():
        D.upload(k, v)
    return {k: np.asarray(D[k], np.float64) for k in hc.FIELDS}


def enable_all(D, down, ddist, area, p, nsub, shade, withdraw=False):
    D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
    if withdraw:
        D.routing_set_withdrawal(True)
    D.routing_kinematic_enable(p)
    D.routing_heat_enable(hc.SUBLEV, shade)


_ctx = functools.partial(rv.context, cell_map=hc.heat_map)


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("withdraw", [False, True], ids=["nowithdrawal", "withdrawal"])
@pytest.mark.parametrize("ncells", [1, 64, 65, 257, 1001])
def test_five_chained_calls_equal_the_restatement(base, ncells, withdraw, lib_path):
    """Per network shape (all seven at 1001 cells, the forest below) and (nsub, dt) with nsub 1, 2 and 5: the scheme and the heat, init with
    the edge values, five calls with a new runoff row and new column fields before each; after every call all fourteen rows against
    routing.kinematic_call(heat=...) on what the device held before it, bit for bit.  At 1001 cells every branch of H1 - H5 is asserted
    on the restatement in every call of the forest's (5, 3600 s) case."""
    D = _ctx(base, lib_path, ncells, withdraw=withdraw)
    ddist, area, p, volr0, wh0, wt0 = hc.cell_values(ncells, 40 + ncells)
    shade, tt0, tr0 = hc.heat_values(ncells, 90 + ncells)
    tab = rt.heat_tables(p, hc.SUBLEV, shade)
    bytes0 = D.device_bytes
    qs = [set_runoff(D, hc.snwcp(c)) for c in range(3)]  # (three runoff rows and three sets of columns serve the five calls in turn)
    hosts = [host_inputs(D, q, area) for q in qs]
    ptr, col, w = D._map
    preps = [rt.heat_prep(ptr, col, w, set_columns(D, c), tab) for c in range(3)]
    cld = (ncells + 63) // 64 * 64
    nets = hc.networks(ncells, 52 + ncells)
    if ncells != 1001:
        nets = {k: nets[k] for k in (("forest",) if ncells >= 3 else ("outlets",))}
    widths = set()
    for name, down in nets.items():
        up = rt.upstream_map(down)
        widths.add(rt.npad_of(up))  # the NPAD the launch picks its kernel by
        for nsub, dt in hc.CASES:
            bytes1 = None
            D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
            if withdraw:
                D.routing_set_withdrawal(True)
            D.routing_kinematic_enable(p)
            bytes1 = D.device_bytes
            D.routing_heat_enable(hc.SUBLEV, shade)
            assert D.device_bytes - bytes1 >= (18 + 1) * 8 * cld
            assert bits(D.routing_read(rt.TT)) == bits(np.full(ncells, rt.TFRZ)) == bits(D.routing_read(rt.TR)) and not D.routing_read(rt.HEAT).any()
            D.routing_init(volr0)
            D.routing_kinematic_init(wh0, wt0)
            D.routing_heat_init(tt0, tr0)
            volr, wh, wt, tt, tr, qsum = volr0, wh0, wt0, tt0, tr0, np.zeros(ncells)
            census_case = ncells == 1001 and name == "forest" and (nsub, dt) == hc.CENSUS_CASE
            for c in range(hc.NCALLS):
                D.upload("qflx_snwcp_liq", hc.snwcp(c % 3))  # the row the call reads is the water balance's of this moment
                D.water_balance(DT)
                set_columns(D, c % 3)
                D.routing(dt)
                qin, qsur, _ = hosts[c % 3]
                census = {} if census_case else None
                heat = {"tab": tab, "prep": preps[c % 3], "tt": tt, "tr": tr, "census": census}
                out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, heat=heat)
                if census_case:
                    assert not hc.missing_branches(census), (c, hc.missing_branches(census))
                wh, wt, volr, qout = out[:4]
                tt, tr = out[4:6]
                with np.errstate(all="ignore"):
                    qsum = rt._canon(qsum + qout)
                want = [volr, qin, qout, qsum, wh, wt, qsur] + list(out[4:])
                for g, h, which in zip(read_rows(D, ROWS), want, ROWS):
                    assert bits(g) == bits(h), (name, nsub, dt, c, NAMES[which], differing(g, h))
                assert D.routing_count() == c + 1
            D.routing_clear()  # frees everything
            assert D.device_bytes == bytes0
    if ncells == 1001:  # (where every shape runs)
        assert widths == {1, 2, 4, 8}, widths  # every instantiation with_npad can pick
    D.close()


# ---- the edge values ---------------------------------------------------------------------------------------------------------------------
def test_the_edge_values_do_what_the_statement_says(base):
    """One call of one sub-step on cells without upstream: the edge values of TT (cells 57 .. 71), TR (74 .. 88), WT (41 .. 55) and VOLR
    (1 .. 15) in cells of their own, PA == 0 in cell 9 and a NaN TA in cell 10: the device equals the restatement, and H9's cases read
    as the header lists them."""
    n, dt = 257, 1800.0
    D = _ctx(base, None, n)
    ddist, area, p, volr0, wh0, wt0 = hc.cell_values(n, 40 + n)
    shade, tt0, tr0 = hc.heat_values(n, 90 + n)
    for c in (hc.PA0_CELL, hc.TANAN_CELL):
        volr0[c], wt0[c], tt0[c], tr0[c] = 4.0e5, 4.0e5, 285.0, 286.0
    wt0[hc.TT_EDGE0:hc.TT_EDGE0 + 16], volr0[hc.TR_EDGE0:hc.TR_EDGE0 + 16] = 4.0e5, 4.0e5  # the edge temperatures stand in stores that hold water
    tab = rt.heat_tables(p, hc.SUBLEV, shade)
    down = hc.networks(n, 1)["outlets"]
    enable_all(D, down, ddist, area, p, 1, shade)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_heat_init(tt0, tr0)
    q = set_runoff(D, hc.snwcp(0))
    qin, qsur, _ = host_inputs(D, q, area)
    prep = rt.heat_prep(*D._map, set_columns(D, 0), tab)
    D.routing(dt)
    out = rt.kinematic_call(wh0, wt0, volr0, qin, qsur, area, p, rt.upstream_map(down), dt, 1, heat={"tab": tab, "prep": prep, "tt": tt0, "tr": tr0})
    got = dict(zip(ROWS, read_rows(D, ROWS)))
    for which, h in zip(HEAT_ROWS + (rt.WH, rt.WT, rt.VOLR), list(out[4:]) + list(out[:3])):
        assert bits(got[which]) == bits(h), (NAMES[which], differing(got[which], h))
    tt, tr, hadj, hsrf = got[rt.TT], got[rt.TR], got[rt.HADJ], got[rt.HSRF]
    zero, negzero, neg, denorm, big, nan, inf, ninf = (2 * i for i in range(8))  # heat_cases.SPECIAL's order, two cells apart
    wmint, wminr = tab["WMINT"], tab["WMINR"]
    # a NaN or infinite TT or TR in a store that holds water: the temperature comes back to TFRZ, the call's HADJ does not
    for first, t, w0, w1, wmin in ((hc.TT_EDGE0, tt, wt0, got[rt.WT], wmint), (hc.TR_EDGE0, tr, volr0, got[rt.VOLR], wminr)):
        for k in (nan, inf, ninf):
            c = first + k
            assert w0[c] > wmin[c] and w1[c] > wmin[c] and t[c] == rt.TFRZ and np.isnan(hadj[c]), (first, k)
        c = first + big  # 1e300 K: t2 * t2 overflows, phi = -inf, the store is held at TFRZ and HADJ is +inf
        assert t[c] == rt.TFRZ and hadj[c] == INF
    # a NaN, zero, negative or denormal WT or VOLR is not > wmin: where the new storage is not either, the store takes TEQ
    seen = 0
    for first, t, w0, w1, wmin in ((41, tt, wt0, got[rt.WT], wmint), (1, tr, volr0, got[rt.VOLR], wminr)):
        for k in (zero, negzero, neg, denorm, nan):
            c = first + k
            assert not (w0[c] > wmin[c])
            if not (w1[c] > wmin[c]):
                seen += 1
                assert t[c] == prep["TEQ"][c], (first, k)
        assert np.isnan(w1[first + nan]) and np.isnan(hadj[first + nan])
    assert seen >= 2
    # PA == 0: qs is finite and negative, the cell's rows are finite; a NaN TA: TEQ = TFRZ, phi NaN, the stores come back to TFRZ
    c = hc.PA0_CELL
    assert prep["PA"][c] == 0.0 and np.isfinite([tt[c], tr[c], hsrf[c], hadj[c]]).all() and hsrf[c] != 0.0
    c = hc.TANAN_CELL
    assert np.isnan(prep["TA"][c]) and prep["TEQ"][c] == rt.TFRZ and tt[c] == rt.TFRZ == tr[c] and np.isnan(hsrf[c]) and np.isnan(hadj[c])
    # the cell without terms exchanges nothing through its surface
    assert not prep["terms"][0] and hsrf[0] == 0.0
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING


@pytest.fixture(scope="module")
def run_base():
    return rv.run_case(heat=True)


_run_context = functools.partial(rv.run_context, parts=("routing", "kinematic", "heat"))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the flag and the extension on against the stepwise calls in every field and row; then a second run (on
    the captured step when the graph is on); the extension switched off between two runs, which drops the captured step and runs the
    form without it, and on again."""
    steps = schedule(2 * NSTEPS)
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:3], FLAGS)
    B.run(DT, steps[:3], FLAGS)
    a = river_snapshot(A, ROWS)
    assert_same(river_snapshot(B, ROWS), a)
    assert np.isfinite(a["route"]).all() and (a["route"][7] != rt.TFRZ).any() and a["route"][10].any() and a["route"][11].any()
    stepwise(A, run_base["rec"], steps[3:NSTEPS], FLAGS)
    B.run(DT, steps[3:NSTEPS], FLAGS)
    assert_same(river_snapshot(B, ROWS), river_snapshot(A, ROWS))
    tt, tr = A.routing_read(rt.TT), A.routing_read(rt.TR)
    for X in (A, B):
        X.routing_heat_clear()
    stepwise(A, run_base["rec"], steps[NSTEPS:NSTEPS + 2], FLAGS)
    B.run(DT, steps[NSTEPS:NSTEPS + 2], FLAGS)
    assert_same(river_snapshot(B, KW_ROWS), river_snapshot(A, KW_ROWS))
    for X in (A, B):
        X.routing_heat_enable(hc.SUBLEV, run_base["shade"])
        X.routing_heat_init(tt, tr)
    stepwise(A, run_base["rec"], steps[NSTEPS + 2:NSTEPS + 5], FLAGS)
    B.run(DT, steps[NSTEPS + 2:NSTEPS + 5], FLAGS)
    assert_same(river_snapshot(B, ROWS), river_snapshot(A, ROWS))
    for X in (A, B):
        X.close()


# ---- 3. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it the routing's rows, TT and TR through elmk_routing_read; a fresh context,
    restart_load and the three _init calls, three more steps: the bits of six steps in one context on all fourteen rows.  The image
    is the one a context without the extension saves."""
    steps = schedule(NSTEPS)
    A = _run_context(run_base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, ROWS)
    size_a = A.restart_size()
    A.close()
    B = _run_context(run_base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    img, count = B.restart_save(), B.routing_count()
    volr, qsum, wh, wt, tt, tr = read_rows(B, (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.TT, rt.TR))
    assert count == 3 and B.restart_size() == size_a
    B.close()
    Cx = _run_context(run_base, True, lib_path, init=False)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.routing_kinematic_init(wh, wt)
    Cx.routing_heat_init(tt, tr)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, ROWS), want)
    # heat_init leaves the other entries' rows alone, and without rows gives TT = TR = TFRZ and zero diagnostics
    Cx.routing_heat_init()
    assert bits(Cx.routing_read(rt.TT)) == bits(np.full(NCELL, rt.TFRZ)) == bits(Cx.routing_read(rt.TR))
    assert not any(Cx.routing_read(w).any() for w in HEAT_ROWS[2:]) and bits(Cx.routing_read(rt.VOLR)) == bits(want["route"][0])
    N = _run_context(run_base, True, lib_path, parts=("routing", "kinematic"))
    assert N.restart_size() == size_a
    N.close()
    Cx.close()


def test_restart_3_plus_3_through_a_version_8_image(run_base):
    """Under ELMK_OPT_RESTART_CELLS a context with the heat saves version 8: version 6 plus the cell sections TT and TR after WT.  3 + 3
    steps through the image with no _read / _init pair give the bits of 6.  The image loads only into a context with the same stages
    on - a version-8 image is refused by a context without the heat and a version-6 image by one with it, with everything untouched;
    a context without the heat saves version 6, byte for byte what it saved before, and with the option off the image is the one it
    always was; restart.py refuses version 8."""
    from elmkernels_amd import restart as R
    steps = schedule(NSTEPS)
    A = _run_context(run_base, True)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, ROWS)
    size_off = A.restart_size()
    A.close()
    P = _run_context(run_base, True, parts=("routing", "kinematic"))  # a context that never had the extension
    P.set_option(st.OPT_RESTART_CELLS, 1)
    P.run(DT, steps[:3], FLAGS)
    img_plain = P.restart_save()
    B = _run_context(run_base, True)
    B.set_option(st.OPT_RESTART_CELLS, 1)
    B.run(DT, steps[:3], FLAGS)
    img = B.restart_save()
    head = np.frombuffer(img[:R.HEADER.itemsize].tobytes(), R.HEADER)[0]
    assert int(head["version"]) == R.VERSION_HEAT == 8 and img.size > size_off
    nsec, hb = int(head["nsections"]), int(head["header_bytes"])
    off = R.HEADER.itemsize + 16 + int(head["nentries"]) * R.ENTRY.itemsize
    table = np.frombuffer(img[off:off + nsec * R.SECTION.itemsize].tobytes(), R.SECTION)
    cells = table[table["kind"] == R.ROUTING_SECTION]
    assert cells["id"].tolist() == [rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.TT, rt.TR] and (cells["extent"] == NCELL).all() and off + table.nbytes <= hb
    for call in (lambda: R.parse(img), lambda: R.merge([img]), lambda: R.slice(img, 0, 5)):
        with pytest.raises(R.RestartError, match="format version"):
            call()
    B.routing_heat_clear()
    img6 = B.restart_save()
    assert int(R.verify(img6)["header"]["version"]) == R.VERSION_ROUTING and bits(img6) == bits(img_plain)
    B.close()
    state_p = river_snapshot(P, KW_ROWS)
    with pytest.raises(L.ElmkError, match="the stream temperature"):
        P.restart_load(img)  # version 8 into a context without the heat
    assert_same(river_snapshot(P, KW_ROWS), state_p)
    P.close()
    Cx = _run_context(run_base, True, init=False)
    Cx.set_option(st.OPT_RESTART_CELLS, 1)
    state_c = river_snapshot(Cx, ROWS)
    with pytest.raises(L.ElmkError, match="the stream temperature"):
        Cx.restart_load(img6)  # version 6 into a context with it
    assert_same(river_snapshot(Cx, ROWS), state_c)
    Cx.restart_load(img)
    assert Cx.routing_count() == 3 and not any(Cx.routing_read(w).any() for w in HEAT_ROWS[2:])
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, ROWS), want)
    Cx.set_option(st.OPT_RESTART_CELLS, 0)
    assert Cx.restart_size() == size_off
    Cx.close()


def test_a_row_on_a_history_tape(run_base):
    """elmk_cell_history_add_row over TR (AVG and MAX) while the extension is on equals history.fold_cell_rows over the rows read after
    each call; while an entry exists elmk_routing_heat_clear is refused and changes nothing."""
    D = _run_context(run_base, False)
    ids = {op: D.cell_history_add_row(0, "routing", rt.TR, op) for op in ("avg", "max")}
    samples = []
    for c in range(3):
        set_runoff(D, hc.snwcp(c)[:NCOL])
        set_columns(D, c, NCOL)
        D.routing(DT)
        D.history_accumulate()
        samples.append(D.routing_read(rt.TR))
    assert bits(samples[0]) != bits(samples[2])
    for op, e in ids.items():
        assert bits(D.history_read(e, n=NCELL)) == bits(hs.fold_cell_rows(op, samples)), op
    bytes1 = D.device_bytes
    with pytest.raises(L.ElmkError, match="elmk_history_clear first"):
        D.routing_heat_clear()
    assert D.device_bytes == bytes1 and bits(D.routing_read(rt.TR)) == bits(samples[-1])
    D.history_clear()
    D.routing_heat_clear()
    with pytest.raises(L.ElmkError, match="row out of range"):
        D.cell_history_add_row(0, "routing", rt.TR, "avg")
    D.close()


# ---- 4. the clear ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_clear_returns_to_the_scheme_without_temperatures(base, lib_path):
    """Three calls with the extension, heat_clear, two calls without: on every water row the bits of a context that never had it, all
    the way (H8).  While it is on kinematic_clear is refused and changes nothing."""
    n = 257
    ddist, area, p, volr0, wh0, wt0 = hc.cell_values(n, 40 + n)
    shade, tt0, tr0 = hc.heat_values(n, 90 + n)
    down = hc.networks(n, 52 + n)["forest"]
    A, B = _ctx(base, lib_path, n), _ctx(base, lib_path, n)
    bytes0 = A.device_bytes
    for D in (A, B):
        D.routing_enable(down, ddist, area, rt.EFFVEL, 3)
        D.routing_kinematic_enable(p)
        set_runoff(D, hc.snwcp(0))
        set_columns(D, 0)
        D.routing_init(volr0)
        D.routing_kinematic_init(wh0, wt0)
    bytes1 = A.device_bytes
    A.routing_heat_enable(hc.SUBLEV, shade)
    bytes2 = A.device_bytes
    A.routing_heat_init(tt0, tr0)
    for _ in range(3):
        for D in (A, B):
            D.routing(1800.0)
    held = read_rows(A, KW_ROWS)
    for g, h in zip(held, read_rows(B, KW_ROWS)):
        assert bits(g) == bits(h)  # H8: the water never saw the heat
    with pytest.raises(L.ElmkError, match="elmk_routing_heat_clear first"):
        A.routing_kinematic_clear()
    assert A.device_bytes == bytes2
    A.routing_heat_clear()
    A.routing_heat_clear()  # nothing to free: OK
    assert A.device_bytes == bytes1 == B.device_bytes and A.routing_count() == 3
    for w in HEAT_ROWS:
        with pytest.raises(L.ElmkError, match="unknown row"):
            A.routing_read(w)
    for _ in range(2):
        for D in (A, B):
            D.routing(1800.0)
    for g, h in zip(read_rows(A, KW_ROWS), read_rows(B, KW_ROWS)):
        assert bits(g) == bits(h)
    v = A.routing_read(rt.VOLR)
    A.routing_heat_enable(0, None)  # ... and on again: TT and TR come back at TFRZ, the water stays
    assert bits(A.routing_read(rt.TT)) == bits(np.full(n, rt.TFRZ)) and bits(A.routing_read(rt.VOLR)) == bits(v)
    A.routing(1800.0)
    A.routing_clear()  # frees everything
    assert A.device_bytes == bytes0
    B.routing_kinematic_clear()
    B.routing_clear()
    assert B.device_bytes == bytes0
    A.close()
    B.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(run_base):
    """Every refusal of the four entries and of the interlocks, in both directions, with nothing changed by any."""
    b, rows_, m, down, ddist, area, p, volr, wh, wt, shade = (run_base[k] for k in ("b", "rows", "map", "down", "ddist", "area", "p", "volr", "wh", "wt", "shade"))
    tt, tr = run_base["temps"]

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    enable = lambda sub=hc.SUBLEV, s=shade: D.routing_heat_enable(sub, s)  # noqa: E731
    D = _new(b[0], b[1], b[2], rows_, None, b[3], b[4])
    D.set_graph(True)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    bytes0, size0 = D.device_bytes, D.restart_size()
    refused(enable, D.routing_heat_init, D.routing_heat_budget, match="not enabled")
    D.routing_heat_clear()  # nothing to free: OK
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr)
    refused(enable, D.routing_heat_init, D.routing_heat_budget, match="the scheme is not on")
    D.routing_kinematic_enable(p)
    D.routing_kinematic_init(wh, wt)
    bytes1 = D.device_bytes
    state1 = river_snapshot(D, KW_ROWS)
    refused(D.routing_heat_init, D.routing_heat_budget, match="the extension is not on")
    refused(*(lambda w=w: D.routing_read(w) for w in HEAT_ROWS), lambda: D.routing_read(20), match="unknown row")
    refused(lambda: enable(sub=-1), lambda: enable(sub=15), match=r"elmk_routing_heat_enable: sublev outside 0 \.\. 14$")
    for v in (-1.0e-9, 1.0 + 1.0e-9, NAN, INF, -INF):
        s = shade.copy()
        s[11] = v
        s[40] = NAN
        refused(lambda s=s: enable(s=s), match=r"elmk_routing_heat_enable: SHADE outside \[0, 1\] at cell 11$")
    sp = np.ascontiguousarray(shade).ctypes.data_as(C.c_void_p)
    with captured(D) as cap_:
        rc_ = D.lib.elmk_routing_heat_enable(D.ctx, 0, sp)
        cap_.end()
        assert rc_ == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    with pytest.raises(ValueError):
        enable(s=shade[:-1])
    refused(lambda: D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, rt.TR, st.HIST_AVG), match="row out of range")
    # the interlock, one way: the heat is refused while the inundation or the reservoirs are on
    rdepth, eprof = np.full(NCELL, 2.0), np.repeat(np.arange(11.0)[:, None], NCELL, axis=1)
    D.routing_inundation_enable(rdepth, eprof)
    refused(enable, match="elmk_routing_heat_enable: the floodplain inundation is on .elmk_routing_inundation_clear first.$")
    D.routing_inundation_clear()
    dam = (np.where(np.arange(NCELL) % 7 == 3, 1.0e9, 0.0), np.full((12, NCELL), 20.0), np.full(NCELL, 0.5), np.zeros(NCELL, np.int32))
    D.routing_reservoir_enable(*dam)
    refused(enable, match="elmk_routing_heat_enable: the reservoirs are on .elmk_routing_reservoir_clear first.$")
    D.routing_reservoir_clear()
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(river_snapshot(D, KW_ROWS), state1)

    enable()
    bytes2 = D.device_bytes
    assert bytes2 > bytes1 and D.restart_size() == size0  # the image is what it was
    D.routing_heat_init(tt, tr)
    state2 = river_snapshot(D, ROWS)
    refused(enable, match="already on")
    refused(D.routing_kinematic_clear, match="elmk_routing_heat_clear first")
    # ... and the other way: the inundation's and the reservoirs' enables are refused while the heat is on
    refused(lambda: D.routing_inundation_enable(rdepth, eprof), match="elmk_routing_inundation_enable: the stream temperature is on .elmk_routing_heat_clear first.$")
    refused(lambda: D.routing_reservoir_enable(*dam), match="elmk_routing_reservoir_enable: the stream temperature is on .elmk_routing_heat_clear first.$")
    refused(lambda: D.routing_read(20), lambda: D.routing_read(-1), lambda: D.routing_read(rt.WF), lambda: D.routing_read(rt.RES),
            lambda: D.routing_read(rt.TT, cell0=NCELL, n=1))
    refused(lambda: D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, 20, st.HIST_AVG), match="row out of range")
    with pytest.raises(ValueError):
        D.routing_heat_init(np.zeros(NCELL + 1))
    assert D.lib.elmk_routing_heat_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap_:
        rcs = (D.lib.elmk_routing_heat_clear(D.ctx), D.lib.elmk_routing_heat_init(D.ctx, None, None), D.lib.elmk_routing_heat_budget(D.ctx, sp))
        cap_.end()
        assert rcs == (-1, -1, -1) and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes2 and D.restart_size() == size0
    assert_same(river_snapshot(D, ROWS), state2)
    # the following call is the call of a context that met no refusal
    W = _run_context(run_base, True, nsub=2)
    for X in (D, W):
        set_runoff(X, hc.snwcp(0)[:NCOL])
        X.routing(DT)
    for g, h in zip(read_rows(D, ROWS), read_rows(W, ROWS)):
        assert bits(g) == bits(h)
    D.routing_heat_clear()
    assert D.device_bytes == bytes1
    enable()
    D.routing_clear()  # frees everything
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    refused(enable, match="not enabled")
    D.close()
    W.close()


# ---- the budget ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [1, 65, 1001])
def test_budget_equals_the_restatement(base, ncells):
    D = _ctx(base, None, ncells)
    ddist, area, p, volr0, wh0, wt0 = hc.cell_values(ncells, 40 + ncells)
    volr0, wh0, wt0 = (finite(x) for x in (volr0, wh0, wt0))
    shade, tt0, tr0 = hc.heat_values(ncells, 90 + ncells)
    tt0, tr0 = (np.where((x > 200.0) & (x < 400.0), x, 280.0) for x in (tt0, tr0))
    down = hc.networks(ncells, 5)["forest" if ncells >= 3 else "outlets"]
    enable_all(D, down, ddist, area, p, 2, shade)
    D.routing_init(volr0 + (1.0e5 if ncells == 1 else 0.0))
    D.routing_kinematic_init(wh0, wt0)
    D.routing_heat_init(tt0, tr0)
    q = hc.snwcp(1)
    q[9] = 2.0e-5
    set_runoff(D, q)
    for k, v in hc.columns(hc.NCOLS, 77, 1, edges=False).items():
        D.upload(k, v)
    for _ in range(2):
        D.routing(1800.0)
    rows = read_rows(D, ROWS)
    want, want_kw = rt.budget(rows[0], rows[1], rows[2], down), rt.kinematic_budget(rows[4], rows[5])
    want_heat = rt.heat_budget(*rows[9:], down)
    assert np.isfinite(want_heat).all() and want_heat[0] > 0.0 and want_heat[4] != 0.0
    for _ in range(2):  # (in turn: the three share the reduction's scratch)
        assert bits(D.routing_heat_budget()) == bits(want_heat)
        assert bits(D.routing_kinematic_budget()) == bits(want_kw)
        assert bits(D.routing_budget()) == bits(want)
    for g, h in zip(read_rows(D, ROWS), rows):
        assert bits(g) == bits(h)  # (the calls change no row)
    D.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_heat_demo(tmp_path):
    """examples/heat_demo.cc builds with g++ against the C ABI and runs: a summer day on a short chain, a cold tributary joining a warm
    river; below the confluence the river is colder than above it and warmer than the tributary, and the day's budget closes."""
    out = run_demo(build_demo("heat_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(48))
    above, trib, below = (np.array([float(s[k]) for s in steps]) for k in (1, 2, 3))
    assert (trib[-24:] < below[-24:]).all() and (below[-24:] < above[-24:]).all()
    assert all(rt.TFRZ <= x.min() and x.max() <= rt.TMAX for x in (above, trib, below))
    assert sum(s.startswith("budget: closes to") for s in out) == 1
