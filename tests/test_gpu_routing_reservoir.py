"""Reservoirs on the device (include/elmk.h "reservoirs"): the DAM form of k_kinematic_prep and k_kinematic_step against the host
restatement (routing.kinematic_call(dam=...)) bit for bit on all thirteen rows, in both builds, over five chained calls on every
network shape, size, nsub and dt, plain and flood, the withdrawal on and off, with the edge values in RES and CAP cells of their own;
the stage inside elmk_run across a month boundary against the stepwise calls with elmk_routing_reservoir_time, graph on and off;
restarts through _read and _init and through a version-7 image; the rows on a history tape; the clear; the river supply limit's D7;
every refusal; the budget; the example."""
import ctypes as C
import functools

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc
from tests import reservoir_cases as rc
from tests import river_cases as rv
from tests.hydrology_cases import _new, prepare
from tests.irrigation_cases import generated, smpso_of
from tests.river_cases import NCELL, NCOL, NSTEPS, TOL, differing, finite, host_inputs, read_rows, river_snapshot, set_runoff
from tests.run_cases import DT, NREC, assert_same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

KW_ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR)
FP_ROWS = (rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC)
DAM_ROWS = (rt.RES, rt.KRLS, rt.RES_TAKE)
NAMES = {rt.VOLR: "VOLR", rt.QIN: "QIN", rt.QOUT: "QOUT", rt.QOUT_SUM: "QOUT_SUM", rt.WH: "WH", rt.WT: "WT", rt.QSUR: "QSUR", rt.WF: "WF",
         rt.FLOOD_DEPTH: "FLOOD_DEPTH", rt.FLOOD_FRAC: "FLOOD_FRAC", rt.RES: "RES", rt.KRLS: "KRLS", rt.RES_TAKE: "RES_TAKE"}
NAN, INF = rc.NAN, rc.INF


def rows_of(flood):
    return KW_ROWS + (FP_ROWS if flood else ()) + DAM_ROWS


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return rv.base()


_ctx = functools.partial(rv.context, cell_map=ic.cell_map)


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("withdraw", [False, True], ids=["nowithdrawal", "withdrawal"])
@pytest.mark.parametrize("flood", [False, True], ids=["plain", "flood"])
@pytest.mark.parametrize("ncells", [1, 64, 65, 257, 1001])
def test_five_chained_calls_equal_the_restatement(base, ncells, flood, withdraw, lib_path):
    """Per network shape and (nsub, dt): the scheme, the reservoirs and (flood) the inundation, init with the edge values, five calls in
    months 0 .. 4 with `begins` on call 3 and a new runoff row before each; after every call all thirteen rows (ten without the
    inundation) against routing.kinematic_call(dam=...) on what the device held before it, bit for bit.  The next call starts from
    the flow that VOLR, RES and KRLS of this one give, so the chain covers it.  At 1001 cells every branch of D1 - D3 and D2 is
    asserted on the restatement in every call of the forest's (3, 1800 s) case."""
    D = _ctx(base, lib_path, ncells, withdraw=withdraw)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    cap, target, beta, mstart, res0, krls0 = rc.dam_values(ncells, 90 + ncells)
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    bytes0 = D.device_bytes
    qs = [set_runoff(D, ic.snwcp(c)) for c in range(3)]  # (three runoff rows serve the five calls in turn)
    hosts = [host_inputs(D, q, area) for q in qs]
    cld = (ncells + 63) // 64 * 64
    rows, widths = rows_of(flood), set()
    for name, down in ic.networks(ncells, 52 + ncells).items():
        up = rt.upstream_map(down)
        widths.add(rt.npad_of(up))  # the NPAD the launch picks its kernel by
        for nsub, dt in ic.CASES:
            rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(ncells, 60 + ncells, area, p0, volr0, wh0, wt0, nsub, dt)
            ftab = rt.inundation_tables(area, p, rdepth, eprof) if flood else None
            D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
            if withdraw:
                D.routing_set_withdrawal(True)
            D.routing_kinematic_enable(p)
            if flood and nsub != 3:  # (either order)
                D.routing_inundation_enable(rdepth, eprof)
            bytes2 = D.device_bytes
            D.routing_reservoir_enable(cap, target, beta, mstart)
            assert D.device_bytes - bytes2 >= (4 + 16) * 8 * cld + 4 * cld
            if flood and nsub == 3:
                D.routing_inundation_enable(rdepth, eprof)
            assert bits(D.routing_read(rt.KRLS)) == bits(np.ones(ncells)) and not D.routing_read(rt.RES).any() and not D.routing_read(rt.RES_TAKE).any()
            D.routing_init(volr)
            D.routing_kinematic_init(wh, wt)
            if flood:
                D.routing_inundation_init(wf)
            D.routing_reservoir_init(res0, krls0)
            res, krls, qsum = res0, krls0, np.zeros(ncells)
            census = ncells == 1001 and name == "forest" and (nsub, dt) == (3, 1800.0)
            for c in range(rc.NCALLS):
                D.upload("qflx_snwcp_liq", ic.snwcp(c % 3))  # the row the call reads is the water balance's of this moment
                D.water_balance(DT)
                month, begins = rc.call_time(c)
                D.routing_reservoir_time(month, begins)
                D.routing(dt)
                qin, qsur, wd = hosts[c % 3]
                dam = {"tab": tab, "res": res, "krls": krls, "month": month, "begins": begins, "withdrawal": wd}
                if census:
                    seen = rc.call_census(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, dam, flood=(ftab, wf) if flood else None)
                    missing = [k for k in rt.DAM_BRANCHES[:7 if not withdraw else 9] if not seen[k].any()]
                    assert not missing and seen["D1"].any() == begins, (c, missing)
                out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, flood=(ftab, wf) if flood else None, dam=dam)
                wh, wt, volr, qout = out[:4]
                res, krls, take, qin1 = out[-4:]
                with np.errstate(all="ignore"):
                    qsum = rt._canon(qsum + qout)
                want = [volr, qin1, qout, qsum, wh, wt, qsur]
                if flood:
                    wf = out[4]
                    want += [wf, out[5], out[6]]
                want += [res, krls, take]
                for g, h, which in zip(read_rows(D, rows), want, rows):
                    assert bits(g) == bits(h), (name, nsub, dt, c, NAMES[which], differing(g, h))
                assert D.routing_count() == c + 1
            if not withdraw:
                assert not take.any()
            elif ncells >= 64:
                assert (take[tab["DAM"]] > 0.0).any() and not take[~tab["DAM"]].any()
            D.routing_clear()  # frees everything
            assert D.device_bytes == bytes0
    if ncells >= 63:
        assert widths == {1, 2, 4, 8}, widths  # every instantiation with_npad can pick
    D.close()


# ---- the edge values ---------------------------------------------------------------------------------------------------------------------
def test_the_edge_values_do_what_the_statement_says(base):
    """One call of one sub-step on cells without upstream: RES's edge values (dams of cells 59, 61 .. 73, BETA 0.6, TARGET 50) and CAP's
    (cells 75 .. 81), by kind, as D8 lists them."""
    n, dt = 257, 1800.0
    D = _ctx(base, None, n)
    ddist, area, p, volr0, wh0, wt0 = ic.cell_values(n, 40 + n)
    cap, target, beta, mstart, res0, krls0 = rc.dam_values(n, 90 + n)
    e0 = rc.RES_EDGE0
    volr0[e0:e0 + 24] = 4.0e5
    D.routing_enable(ic.networks(n, 1)["outlets"], ddist, area, rt.EFFVEL, 1)
    D.routing_kinematic_enable(p)
    D.routing_reservoir_enable(cap, target, beta, mstart)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_reservoir_init(res0, krls0)
    set_runoff(D, ic.snwcp(0))
    D.routing_reservoir_time(rc.BEGINS_CALL, True)  # these cells' MSTART: D1 for all of them
    D.routing(dt)
    res, krls, qout = D.routing_read(rt.RES), D.routing_read(rt.KRLS), D.routing_read(rt.QOUT)
    e = rt.channel_flow(volr0, p[rt.RLEN], p[rt.RWIDTH], rt.kinematic_params(p)[2], dt)
    at = {v if v == v else "nan": e0 + 2 * i for i, v in enumerate(rc.SPECIAL)}
    assert (e[e0:e0 + 24] > 0.0).all()
    # zero, negative zero, negative and the denormal: RES <= SMIN, nothing is drawn; KRLS = RES / C85 of that RES
    for v in (0.0, -3.5e4, 5e-324):
        c = at[v]
        assert krls[c] == v / (0.85 * 1.0e9) and e[c] * 0.1 <= qout[c] <= e[c] and res[c] == v + (e[c] - qout[c]) * dt, (v, c)
    c = at[1e300]  # above CAP at once: spills what it holds over CAP, which is 1e300
    assert res[c] == 1.0e9 and qout[c] > 1e296 and krls[c] == 1e300 / (0.85 * 1.0e9)
    c = at["nan"]
    assert np.isnan(res[c]) and np.isnan(krls[c]) and np.isnan(qout[c])
    c = at[INF]  # D1's KRLS = +inf makes q and eo +inf, and s = inf - inf
    assert np.isnan(res[c]) and qout[c] == INF and krls[c] == INF
    c = at[-INF]  # q = 0.6 * (-inf * 50) + 0.4 e = -inf is floored to 0.1 e; the reservoir stays where it is
    assert res[c] == -INF and krls[c] == -INF and qout[c] == 0.1 * e[c]
    # CAP's edge values: 0.0 and -0.0 are no dams (nothing is written); 5e-324 is a dam without dead storage whose D1 gives KRLS = +inf,
    # so that it draws all it holds; 1e300 holds everything
    c0 = rc.CAP_EDGE0
    assert res[c0] == 1.0e5 and res[c0 + 2] == 1.0e5 and krls[c0] == 1.0 and qout[c0] == e[c0] and qout[c0 + 2] == e[c0 + 2]
    assert abs(res[c0 + 4]) < 1.0e-6 and krls[c0 + 4] == INF and qout[c0 + 4] == e[c0 + 4] + 1.0e5 / dt
    assert krls[c0 + 6] == 1.0e5 / (0.85 * 1e300) and res[c0 + 6] > 1.0e5 and qout[c0 + 6] < e[c0 + 6]
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING


def month_schedule(nsteps):
    """run_cases.schedule moved to the end of January: half-hour steps from 22:30 of day 30, so that step 3 starts at 00:00 of
    1 February."""
    S = schedule(nsteps)
    for s in range(nsteps):
        ddoy = 30.9375 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"] = ddoy + 1.0, int(ddoy)
    return S


@pytest.fixture(scope="module")
def run_base():
    return rv.run_case(dam=True)


_run_context = functools.partial(rv.run_context, parts=("routing", "kinematic", "inundation", "reservoir"))


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise_across_a_month_boundary(run_base, graph):
    """Six steps of elmk_run from 22:30 of 31 January with the flag and the extension on against the stepwise calls with
    elmk_routing_reservoir_time in every field and row: step 3 begins February, which sets KRLS in the dams whose year begins then and
    changes every dam's target.  Then a second run (on the captured step when the graph is on); the extension switched off between
    two runs, which drops the captured step and runs the form without it, and on again."""
    steps = month_schedule(2 * NSTEPS)
    cap, target, beta, mstart, res0, krls0 = run_base["dam"]
    rows = rows_of(True)
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:3], FLAGS, reservoir_time=True)
    B.run(DT, steps[:3], FLAGS)
    a = river_snapshot(A, rows)
    assert_same(river_snapshot(B, rows), a)
    assert bits(a["route"][11]) == bits(krls0)  # January: no D1
    stepwise(A, run_base["rec"], steps[3:NSTEPS], FLAGS, reservoir_time=True)
    B.run(DT, steps[3:NSTEPS], FLAGS)
    a = river_snapshot(A, rows)
    assert_same(river_snapshot(B, rows), a)
    dams = rc.dam_cells(NCELL)
    moved = a["route"][11] != krls0
    assert moved[dams[::2]].all() and not moved[dams[1::2]].any() and B.routing_count() == NSTEPS
    # the month matters: a context that stays in January ends elsewhere
    J = _run_context(run_base, False)
    for s in range(NSTEPS):
        steps_j = steps[s:s + 1].copy()
        steps_j["doy"], steps_j["decday"] = 13, 14.5
        J.run(DT, steps_j, FLAGS)
    assert bits(J.routing_read(rt.RES)) != bits(a["route"][10]) and bits(J.routing_read(rt.KRLS)) == bits(krls0)
    J.close()
    stepwise(A, run_base["rec"], steps[NSTEPS:], FLAGS, reservoir_time=True)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(river_snapshot(B, rows), river_snapshot(A, rows))
    res, krls = A.routing_read(rt.RES), A.routing_read(rt.KRLS)
    for X in (A, B):
        X.routing_reservoir_clear()
    stepwise(A, run_base["rec"], steps[:2], FLAGS)
    B.run(DT, steps[:2], FLAGS)
    assert_same(river_snapshot(B, rows[:10]), river_snapshot(A, rows[:10]))
    for X in (A, B):
        X.routing_reservoir_enable(cap, target, beta, mstart)
        X.routing_reservoir_init(res, krls)
    stepwise(A, run_base["rec"], steps[2:5], FLAGS, reservoir_time=True)
    B.run(DT, steps[2:5], FLAGS)
    assert_same(river_snapshot(B, rows), river_snapshot(A, rows))
    for X in (A, B):
        X.close()


# ---- 3. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it the routing's rows, RES and KRLS through elmk_routing_read; a fresh context,
    restart_load and the four _init calls, three more steps: the bits of six steps in one context on all thirteen rows.  The image
    is the one a context without the extension saves."""
    steps = month_schedule(NSTEPS)
    rows = rows_of(True)
    A = _run_context(run_base, True, lib_path)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, rows)
    size_a = A.restart_size()
    A.close()
    B = _run_context(run_base, True, lib_path)
    B.run(DT, steps[:3], FLAGS)
    img, count = B.restart_save(), B.routing_count()
    volr, qsum, wh, wt, wf, res, krls = read_rows(B, (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF, rt.RES, rt.KRLS))
    assert count == 3 and B.restart_size() == size_a
    B.close()
    Cx = _run_context(run_base, True, lib_path, init=False)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.routing_kinematic_init(wh, wt)
    Cx.routing_inundation_init(wf)
    Cx.routing_reservoir_init(res, krls)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, rows), want)
    # reservoir_init leaves the other entries' rows alone, and without rows gives RES 0, KRLS 1, RES_TAKE 0
    Cx.routing_reservoir_init()
    assert not Cx.routing_read(rt.RES).any() and not Cx.routing_read(rt.RES_TAKE).any() and bits(Cx.routing_read(rt.KRLS)) == bits(np.ones(NCELL))
    assert bits(Cx.routing_read(rt.VOLR)) == bits(want["route"][0]) and bits(Cx.routing_read(rt.WF)) == bits(want["route"][7])
    N = _run_context(run_base, True, lib_path, parts=("routing", "kinematic", "inundation"))
    assert N.restart_size() == size_a
    N.close()
    Cx.close()


def test_restart_3_plus_3_through_a_version_7_image(run_base):
    """Under ELMK_OPT_RESTART_CELLS a context with the reservoirs saves version 7: version 6 plus the cell sections RES and KRLS after
    WF.  3 + 3 steps through the image with no _read / _init pair give the bits of 6; RES_TAKE comes back zero and is rewritten by the
    next call.  The image loads only into a context with the same stages on; a context without the reservoirs saves version 6, byte
    for byte what it saved before, and with the option off the image is the one it always was; restart.py refuses version 7."""
    from elmkernels_amd import restart as R
    steps = month_schedule(NSTEPS)
    rows = rows_of(True)
    A = _run_context(run_base, True)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, rows)
    size_off = A.restart_size()
    A.close()
    B = _run_context(run_base, True)
    B.set_option(st.OPT_RESTART_CELLS, 1)
    B.run(DT, steps[:3], FLAGS)
    img = B.restart_save()
    head = np.frombuffer(img[:R.HEADER.itemsize].tobytes(), R.HEADER)[0]
    assert int(head["version"]) == R.VERSION_RESERVOIR == 7 and img.size > size_off
    nsec, hb = int(head["nsections"]), int(head["header_bytes"])
    off = R.HEADER.itemsize + 16 + int(head["nentries"]) * R.ENTRY.itemsize
    table = np.frombuffer(img[off:off + nsec * R.SECTION.itemsize].tobytes(), R.SECTION)
    cells = table[table["kind"] == R.ROUTING_SECTION]
    assert cells["id"].tolist() == [rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF, rt.RES, rt.KRLS] and (cells["extent"] == NCELL).all() and off + table.nbytes <= hb
    for call in (lambda: R.parse(img), lambda: R.merge([img]), lambda: R.slice(img, 0, 5)):
        with pytest.raises(R.RestartError, match="format version"):
            call()
    B.routing_reservoir_clear()
    img6 = B.restart_save()
    assert int(R.verify(img6)["header"]["version"]) == R.VERSION_ROUTING
    B.close()
    Cx = _run_context(run_base, True, init=False)
    Cx.set_option(st.OPT_RESTART_CELLS, 1)
    with pytest.raises(L.ElmkError, match="the reservoirs"):
        Cx.restart_load(img6)  # the stages differ
    Cx.restart_load(img)
    assert Cx.routing_count() == 3 and not Cx.routing_read(rt.RES_TAKE).any()
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, rows), want)
    Cx.routing_reservoir_clear()
    with pytest.raises(L.ElmkError, match="the reservoirs"):
        Cx.restart_load(img)
    Cx.set_option(st.OPT_RESTART_CELLS, 0)
    assert Cx.restart_size() == size_off
    Cx.close()


def test_the_rows_on_a_history_tape(run_base):
    """elmk_cell_history_add_row over RES, KRLS and RES_TAKE while the extension is on: the average of three calls is the mean of the
    rows read after each; while an entry exists elmk_routing_reservoir_clear is refused and changes nothing."""
    D = _run_context(run_base, False, parts=("routing", "kinematic", "reservoir"))
    ids = [D.cell_history_add_row(0, "routing", w, st.HIST_AVG) for w in DAM_ROWS]
    got = []
    for c in range(3):
        set_runoff(D, ic.snwcp(c)[:NCOL])
        D.routing_reservoir_time(c, c == 1)
        D.routing(DT)
        D.history_accumulate()
        got.append(read_rows(D, DAM_ROWS))
    for k, e in enumerate(ids):
        acc = -0.0 * np.ones(NCELL)
        for g in got:
            acc = acc + g[k]
        assert bits(D.history_read(e, n=NCELL)) == bits(acc / 3.0), NAMES[DAM_ROWS[k]]
    bytes1 = D.device_bytes
    with pytest.raises(L.ElmkError, match="elmk_history_clear first"):
        D.routing_reservoir_clear()
    assert D.device_bytes == bytes1 and bits(D.routing_read(rt.RES)) == bits(got[-1][0])
    D.history_clear()
    D.routing_reservoir_clear()
    with pytest.raises(L.ElmkError, match="row out of range"):
        D.cell_history_add_row(0, "routing", rt.RES, st.HIST_AVG)
    D.close()


# ---- 4. the clear ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("flood", [False, True], ids=["plain", "flood"])
def test_clear_returns_to_the_free_flowing_channel(base, flood, lib_path):
    """Three calls with the extension, reservoir_clear, two calls without: on the scheme's rows the bits of a context that never had
    it, given the same storages.  While it is on kinematic_clear is refused and changes nothing; the inundation clears independently."""
    n = 257
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(n, 40 + n)
    rdepth, eprof, p, volr0, wh0, wt0, wf0 = ic.flood_values(n, 60 + n, area, p0, volr0, wh0, wt0, 3, 1800.0)
    cap, target, beta, mstart, res0, krls0 = rc.dam_values(n, 90 + n)
    down = ic.networks(n, 52 + n)["forest"]
    rows = KW_ROWS + (FP_ROWS if flood else ())
    A, B = _ctx(base, lib_path, n), _ctx(base, lib_path, n)
    bytes0 = A.device_bytes
    for D in (A, B):
        D.routing_enable(down, ddist, area, rt.EFFVEL, 3)
        D.routing_kinematic_enable(p)
        if flood:
            D.routing_inundation_enable(rdepth, eprof)
        set_runoff(D, ic.snwcp(0))
    bytes1 = A.device_bytes
    A.routing_reservoir_enable(cap, target, beta, mstart)
    bytes2 = A.device_bytes
    A.routing_init(volr0)
    A.routing_kinematic_init(wh0, wt0)
    A.routing_reservoir_init(res0, krls0)
    if flood:
        A.routing_inundation_init(wf0)
    A.routing_reservoir_time(2, False)
    for _ in range(3):
        A.routing(1800.0)
    held = read_rows(A, rows)
    with pytest.raises(L.ElmkError, match="elmk_routing_inundation_clear first" if flood else "elmk_routing_reservoir_clear first"):
        A.routing_kinematic_clear()  # (the inundation's interlock speaks first)
    assert A.device_bytes == bytes2
    for g, h in zip(read_rows(A, rows), held):
        assert bits(g) == bits(h)
    A.routing_reservoir_clear()
    A.routing_reservoir_clear()  # nothing to free: OK
    assert A.device_bytes == bytes1 == B.device_bytes and A.routing_count() == 3
    for g, h in zip(read_rows(A, rows), held):
        assert bits(g) == bits(h)
    for w in DAM_ROWS:
        with pytest.raises(L.ElmkError, match="unknown row"):
            A.routing_read(w)
    B.routing_init(held[0], held[3], 3)
    B.routing_kinematic_init(held[4], held[5])
    if flood:
        B.routing_inundation_init(held[7])
    for _ in range(2):
        for D in (A, B):
            D.routing(1800.0)
    for g, h in zip(read_rows(A, rows), read_rows(B, rows)):
        assert bits(g) == bits(h)
    # ... and on again: RES and RES_TAKE come back zero-filled, KRLS 1.0, VOLR stays; the inundation clears under the reservoirs
    v = A.routing_read(rt.VOLR)
    A.routing_reservoir_enable(cap, target, beta, mstart)
    assert not A.routing_read(rt.RES).any() and bits(A.routing_read(rt.KRLS)) == bits(np.ones(n)) and bits(A.routing_read(rt.VOLR)) == bits(v)
    if flood:
        A.routing_inundation_clear()
        assert bits(A.routing_read(rt.VOLR)) == bits(v) and A.device_bytes < bytes2
        with pytest.raises(L.ElmkError, match="elmk_routing_reservoir_clear first"):
            A.routing_kinematic_clear()
        A.routing(1800.0)
    A.routing_clear()  # frees everything
    assert A.device_bytes == bytes0
    if flood:
        B.routing_inundation_clear()
    B.routing_kinematic_clear()
    B.routing_clear()
    assert B.device_bytes == bytes0
    A.close()
    B.close()


# ---- 5. the river supply limit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_the_supply_limit_counts_the_reservoir(lib_path):
    """D7 (k_irrigation_supply's DAM form) on the shapes of the limit's own device test: 5003 columns over 70 cells, cell 3 with 2100
    columns a dam cell, dams in the empty cell 0, the one-column cell 5, the edge storages' cells 8 .. 13 and every third cell.  Five
    steps of the seven wrappers and elmk_irrigation with the limit behind it; VOLR and RES are set before every step, RES with its
    own edge values and a third of the dams at or below SMIN: RATE and the four cell rows against irrigation.step followed by
    irrigation.supply_limit(dam=), bit for bit, and not what the limit without D7 gives.  After elmk_routing_reservoir_clear the next
    step is S3's again."""
    n, ncells, thr = 5003, 70, 0.1
    cols, scal, soil, sched = generated(n, 900)
    rows0 = prepare(cols, 614)
    m = sc.cell_map(n, ncells, 51, big=(3, 2100), empty=(0, 61, 62, 63, 64, 65, 66), single=(5, 7), free=50)
    ptr, col, w = m
    area, _ = sc.cell_values(ncells, 52)
    cap, target, beta, mstart = rc.supply_dams(ncells, 54, placed=(0, 3, 5, 8, 9, 10, 11, 12, 13))
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    D = _new(cols, scal, soil, rows0, lib_path)
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    D.irrigation_enable(sched)
    D.routing_enable(np.full(ncells, -1, np.int32), np.full(ncells, 5.0e4), area, rt.EFFVEL, 1)
    D.routing_set_withdrawal(True)
    D.routing_kinematic_enable(np.repeat(np.array(ic.BASE)[:, None], ncells, axis=1))
    D.irrigation_supply_enable(thr)
    D.routing_reservoir_enable(cap, target, beta, mstart)
    c = np.arange(n)
    D.irrigation_init(np.where(sched >= 0, 1.0e-4 + 1.0e-6 * (c % 97), 0.0), np.where(c % 3 == 0, (c % 7).astype(np.float64), 0.0))
    smpso = smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    rows, unmet = D.irrigation_rows(), np.zeros(ncells)
    sup_rows = lambda: np.stack([D.irrigation_supply_read(k) for k in (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)])  # noqa: E731
    matters = 0
    for s in range(6):
        tod = (5 * 3600 + 1800 * s) % 86400
        _, volr = sc.cell_values(ncells, 60 + s, lo=2.0 + 0.3 * s, hi=6.0)
        res = rc.supply_res(cap, 70 + s)
        res[3] = (0.05 + 0.2 * s) * cap[3]  # the 2100-column cell: below SMIN in the first step, above it afterwards
        D.routing_init(volr)
        dam = (tab, res)
        if s == 5:
            D.routing_reservoir_clear()
            dam = None
        else:
            D.routing_reservoir_init(res)
        st.timestep7_fused(D, DT)
        fields = {k: D[k] for k in ir.READS}
        _, want = ir.step(fields, rows, sched, DT, tod, smpso, stored=stored)
        want_rate, want_sup = ir.supply_limit(ptr, col, w, area, volr, want[ir.RATE], want[ir.NLEFT], int(DT), thr, unmet,
                                              qflx_irrig=want[ir.QFLX_IRRIG], dam=dam)
        plain_rate, plain_sup = ir.supply_limit(ptr, col, w, area, volr, want[ir.RATE], want[ir.NLEFT], int(DT), thr, unmet,
                                                qflx_irrig=want[ir.QFLX_IRRIG])
        matters += int(bits(want_sup[ir.RATIO]) != bits(plain_sup[ir.RATIO])) + 10 * int(bits(want_rate) != bits(plain_rate))
        D.irrigation(DT, tod)
        rows, sup = D.irrigation_rows(), sup_rows()
        assert bits(rows[ir.RATE]) == bits(want_rate), (s, "RATE", np.nonzero(rows[ir.RATE] != want_rate)[0][:5])
        assert bits(rows[ir.NLEFT]) == bits(want[ir.NLEFT]) and bits(rows[ir.QFLX_IRRIG]) == bits(want[ir.QFLX_IRRIG]), s
        for k in range(4):
            assert bits(sup[k]) == bits(want_sup[k]), (s, "row", k, np.nonzero(sup[k] != want_sup[k])[0][:5])
        if dam is not None:
            assert bits(D.routing_read(rt.RES)) == bits(res)  # (the limit only reads it)
        unmet = sup[ir.UNMET_SUM]
    assert matters % 10 >= 4 and matters >= 10
    D.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(run_base):
    """Every refusal of the five entries and of the interlocks, with nothing changed by any."""
    b, rows_, m, down, ddist, area, rdepth, eprof, p, volr, wh, wt, wf = (run_base[k] for k in ("b", "rows", "map", "down", "ddist", "area", "rdepth", "eprof", "p", "volr", "wh", "wt", "wf"))
    cap, target, beta, mstart, res, krls = run_base["dam"]
    rows = rows_of(False)

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    enable = lambda c=cap, t=target, be=beta, ms=mstart: D.routing_reservoir_enable(c, t, be, ms)  # noqa: E731
    D = _new(b[0], b[1], b[2], rows_, None, b[3], b[4])
    D.set_graph(True)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    bytes0, size0 = D.device_bytes, D.restart_size()
    refused(enable, D.routing_reservoir_init, D.routing_reservoir_budget, lambda: D.routing_reservoir_time(0), match="not enabled")
    D.routing_reservoir_clear()  # nothing to free: OK
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_init(volr)
    refused(enable, D.routing_reservoir_init, D.routing_reservoir_budget, lambda: D.routing_reservoir_time(0), match="the scheme is not on")
    D.routing_kinematic_enable(p)
    D.routing_kinematic_init(wh, wt)
    bytes1 = D.device_bytes
    state1 = river_snapshot(D, KW_ROWS)
    refused(D.routing_reservoir_init, D.routing_reservoir_budget, lambda: D.routing_reservoir_time(0), match="the extension is not on")
    refused(*(lambda w=w: D.routing_read(w) for w in DAM_ROWS), lambda: D.routing_read(13), match="unknown row")
    for v in (-1.0, NAN, INF, -INF):
        c = cap.copy()
        c[11] = v
        refused(lambda c=c: enable(c=c), match="elmk_routing_reservoir_enable: CAP not finite and >= 0 at cell 11$")
    dam = int(rc.dam_cells(NCELL)[2])
    for k in (0, 11):
        for v in (-1.0e-3, NAN, INF):
            t = target.copy()
            t[k, dam] = v
            refused(lambda t=t: enable(t=t), match=f"elmk_routing_reservoir_enable: TARGET not finite and >= 0 at cell {dam}$")
    for v in (-1.0e-9, 1.0 + 1.0e-9, NAN):
        be = beta.copy()
        be[dam] = v
        refused(lambda be=be: enable(be=be), match=rf"elmk_routing_reservoir_enable: BETA outside \[0, 1\] at cell {dam}$")
    for v in (-1, 12):
        ms = mstart.copy()
        ms[dam] = v
        refused(lambda ms=ms: enable(ms=ms), match=rf"elmk_routing_reservoir_enable: MSTART outside 0 \.\. 11 at cell {dam}$")
    arrs = [np.ascontiguousarray(x) for x in (cap, target, beta, mstart)]
    ptrs = [x.ctypes.data_as(C.c_void_p) for x in arrs]
    for k in range(4):
        args = list(ptrs)
        args[k] = None
        assert D.lib.elmk_routing_reservoir_enable(D.ctx, *args) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap_:
        rc_ = D.lib.elmk_routing_reservoir_enable(D.ctx, *ptrs)
        cap_.end()
        assert rc_ == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    for call in (lambda: enable(c=cap[:-1]), lambda: enable(t=target[:, :-1]), lambda: enable(t=target[:-1]), lambda: enable(be=beta[:-1]),
                 lambda: enable(ms=mstart[:-1])):
        with pytest.raises(ValueError):
            call()
    refused(lambda: D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, rt.RES, st.HIST_AVG), match="row out of range")
    assert D.device_bytes == bytes1 and D.restart_size() == size0
    assert_same(river_snapshot(D, KW_ROWS), state1)

    enable()
    bytes2 = D.device_bytes
    assert bytes2 > bytes1 and D.restart_size() == size0  # the image is what it was
    D.routing_reservoir_init(res, krls)
    D.routing_reservoir_time(7, True)
    state2 = river_snapshot(D, rows)
    refused(enable, match="already on")
    refused(D.routing_kinematic_clear, match="elmk_routing_reservoir_clear first")
    refused(lambda: D.routing_reservoir_time(-1), lambda: D.routing_reservoir_time(12), match="month outside 0 .. 11")
    refused(lambda: D.routing_read(13), lambda: D.routing_read(-1), lambda: D.routing_read(rt.WF), lambda: D.routing_read(rt.RES, cell0=NCELL, n=1))
    refused(lambda: D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, 13, st.HIST_AVG), match="row out of range")
    with pytest.raises(ValueError):
        D.routing_reservoir_init(np.zeros(NCELL + 1))
    assert D.lib.elmk_routing_reservoir_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap_:
        rcs = (D.lib.elmk_routing_reservoir_clear(D.ctx), D.lib.elmk_routing_reservoir_init(D.ctx, None, None),
               D.lib.elmk_routing_reservoir_budget(D.ctx, ptrs[0]), D.lib.elmk_routing_reservoir_time(D.ctx, 3, 0))
        cap_.end()
        assert rcs == (-1, -1, -1, -1) and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes2 and D.restart_size() == size0
    assert_same(river_snapshot(D, rows), state2)
    # the following call is the call of a context that met no refusal, in the month and with the `begins` that were set
    W = _run_context(run_base, True, parts=("routing", "kinematic", "reservoir"), nsub=2)
    W.routing_reservoir_time(7, True)
    for X in (D, W):
        set_runoff(X, ic.snwcp(0)[:NCOL])
        X.routing(DT)
    for g, h in zip(read_rows(D, rows), read_rows(W, rows)):
        assert bits(g) == bits(h)
    D.routing_reservoir_clear()
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
    D = _ctx(base, None, ncells, withdraw=True)
    ddist, area, p, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    volr0, wh0, wt0 = (finite(x) for x in (volr0, wh0, wt0))
    cap, target, beta, mstart, res0, krls0 = rc.dam_values(ncells, 90 + ncells)
    res0 = finite(res0)
    down = ic.networks(ncells, 5)["forest" if ncells >= 3 else "outlets"]
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_set_withdrawal(True)
    D.routing_kinematic_enable(p)
    D.routing_reservoir_enable(cap, target, beta, mstart)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_reservoir_init(res0 + (1.0e9 if ncells == 1 else 0.0), krls0)
    q = ic.snwcp(1)
    q[9] = 2.0e-5
    set_runoff(D, q)
    for _ in range(2):
        D.routing(1800.0)
    rows = read_rows(D, rows_of(False))
    want, want_kw, want_dam = rt.budget(rows[0], rows[1], rows[2], down), rt.kinematic_budget(rows[4], rows[5]), rt.reservoir_budget(rows[7], rows[9])
    assert np.isfinite(want_dam).all() and want_dam[0] > 0.0 and (want_dam[1] > 0.0 or ncells == 1)
    for _ in range(2):  # (in turn: the three share the reduction's scratch)
        assert bits(D.routing_reservoir_budget()) == bits(want_dam)
        assert bits(D.routing_kinematic_budget()) == bits(want_kw)
        assert bits(D.routing_budget()) == bits(want)
    for g, h in zip(read_rows(D, rows_of(False)), rows):
        assert bits(g) == bits(h)  # (the calls change no row)
    D.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------
def test_reservoir_demo(tmp_path):
    """examples/reservoir_demo.cc builds with g++ against the C ABI and runs: twelve months with and without the dam, the outlet below
    the dam ranges less widely, the reservoir stays inside [0, CAP]."""
    out = run_demo(build_demo("reservoir_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(96)) and [int(s[1]) for s in steps] == [k // 8 for k in range(96)]
    free, dam, res = (np.array([float(s[k]) for s in steps]) for k in (3, 4, 5))
    assert free.max() > 0.0 and dam.max() > 0.0 and (free >= 0.0).all() and (dam >= 0.0).all() and (res >= 0.0).all() and (res <= 1.0e9).all()
    assert np.ptp(dam[8:]) < np.ptp(free[8:]) and not np.array_equal(free, dam)
    assert sum(s.startswith("dam:    the outlet ranges over") for s in out) == 1
