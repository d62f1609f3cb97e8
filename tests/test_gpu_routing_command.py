"""Command areas on the device (include/elmk.h "command areas"): the CMD form of k_kinematic_prep, k_command_allot and k_command_take
against the host restatement (routing.kinematic_call(dam={..., "command": cmd})) bit for bit on every row, in both builds, over five
chained calls at every size, plain and flood, nsub 1 and 5, with the census at 1001 cells; one dam with 2100 dependents; the edge
values in dams and cells of their own; the stage inside elmk_run against the stepwise calls, graph on and off, the part and the supply
limit switched between runs; restarts through _read and _init and through a version-7 image; the clear; every refusal; the budget; the
river supply limit's CMD form; the rows on a history tape; the example.

k_command_allot takes CMD_DAMS = 64 dams per workgroup and CMD_TILE = 1024 terms per LDS tile: the 1001-cell case has 143 dams (three
workgroups) and the 2300-cell case one dam of 2100 terms (a span of more than two tiles)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import command_cases as cc
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc
from tests import reservoir_cases as rc
from tests import river_cases as rv
from tests.hydrology_cases import _new, prepare
from tests.irrigation_cases import generated, smpso_of
from tests.river_cases import NCELL, NCOL, NSTEPS, TOL, differing, finite, host_inputs, read_rows, river_snapshot, set_runoff
from tests.run_cases import DT, assert_same, schedule, stepwise
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

KW_ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR)
FP_ROWS = (rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC)
DAM_ROWS = (rt.RES, rt.KRLS, rt.RES_TAKE)
CMD_ROWS = (rt.CMD_WANT, rt.CMD_TAKE, rt.CMD_GIVE, rt.CMD_RATIO)
NAMES = {rt.VOLR: "VOLR", rt.QIN: "QIN", rt.QOUT: "QOUT", rt.QOUT_SUM: "QOUT_SUM", rt.WH: "WH", rt.WT: "WT", rt.QSUR: "QSUR", rt.WF: "WF",
         rt.FLOOD_DEPTH: "FLOOD_DEPTH", rt.FLOOD_FRAC: "FLOOD_FRAC", rt.RES: "RES", rt.KRLS: "KRLS", rt.RES_TAKE: "RES_TAKE",
         rt.CMD_WANT: "CMD_WANT", rt.CMD_TAKE: "CMD_TAKE", rt.CMD_GIVE: "CMD_GIVE", rt.CMD_RATIO: "CMD_RATIO"}
NAN, INF = rc.NAN, rc.INF


def rows_of(flood, command=True):
    return KW_ROWS + (FP_ROWS if flood else ()) + DAM_ROWS + (CMD_ROWS if command else ())


@pytest.fixture(scope="module")
def base():
    return rv.base()


_ctx = functools.partial(rv.context, cell_map=cc.cell_map, withdraw=True)


def _enable(D, down, ddist, area, p, nsub, dams, rows, flood=None):
    """The river stage with every part the command areas need, in the order the entry points require."""
    D.routing_enable(down, ddist, area, rt.EFFVEL, nsub)
    D.routing_set_withdrawal(True)
    D.routing_kinematic_enable(p)
    if flood is not None:
        D.routing_inundation_enable(*flood)
    D.routing_reservoir_enable(*dams)
    D.routing_command_enable(*rows)


def _chain(D, ncalls, state, tab, cmd, hosts, area, p, up, dt, nsub, ftab=None, census=None):
    """ncalls chained calls on the device, each against the restatement on what the device held before it, on every row."""
    wh, wt, volr, wf, res, krls = state
    qsum, crow = np.zeros(volr.size), (None, None, None, None)
    rows = rows_of(ftab is not None)
    for c in range(ncalls):
        D.upload("qflx_snwcp_liq", ic.snwcp(c % 3))
        D.water_balance(DT)
        month, begins = rc.call_time(c)
        D.routing_reservoir_time(month, begins)
        D.routing(dt)
        qin, qsur, wd = hosts[c % 3]
        seen = {} if census is not None else None
        command = dict(cmd, take=crow[1], give=crow[2], ratio=crow[3], census=seen)
        dam = {"tab": tab, "res": res, "krls": krls, "month": month, "begins": begins, "withdrawal": wd, "command": command}
        out = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, flood=(ftab, wf) if ftab is not None else None, dam=dam)
        wh, wt, volr, qout = out[:4]
        res, krls, take, qin1 = out[-8:-4]
        crow = out[-4:]
        with np.errstate(all="ignore"):
            qsum = rt._canon(qsum + qout)
        want = [volr, qin1, qout, qsum, wh, wt, qsur]
        if ftab is not None:
            wf = out[4]
            want += [wf, out[5], out[6]]
        want += [res, krls, take, *crow]
        for g, h, which in zip(read_rows(D, rows), want, rows):
            assert bits(g) == bits(h), (nsub, dt, c, NAMES[which], differing(g, h))
        if census is not None:
            census.append(cc.census(cmd, tab, crow[0], seen, crow[3]))
    return crow


# ---- 1. the stage against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("nsub", [1, 5])
@pytest.mark.parametrize("flood", [False, True], ids=["plain", "flood"])
@pytest.mark.parametrize("ncells", [1, 2, 64, 65, 257, 1001])
def test_five_chained_calls_equal_the_restatement(base, ncells, flood, nsub, lib_path):
    """The scheme, the reservoirs, (flood) the inundation and the command areas on the forest (a chain below three cells), init with the
    edge values in the storages, five calls in months 0 .. 4 with `begins` on call 3 and a new runoff row before each; after every
    call all seventeen rows (fourteen without the inundation) against the restatement, bit for bit.  One cell: no term is possible
    and the rows are the reservoir-only context's.  At 1001 cells - 143 dams, three workgroups of k_command_allot - every item of
    the census is asserted on the restatement in every call."""
    dt = 1800.0
    D = _ctx(base, lib_path, ncells)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    cap, target, beta, mstart, res0, krls0 = cc.reservoir_values(ncells, 90 + ncells)
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    qs = [set_runoff(D, ic.snwcp(c)) for c in range(3)]
    hosts = [host_inputs(D, q, area) for q in qs]
    with np.errstate(all="ignore"):
        active = hosts[0][2][1] > 0.0
    rows = cc.command_values(ncells, 3, active)
    cmd = rt.command_tables(cap, *rows)
    down = ic.networks(ncells, 52 + ncells)["forest" if ncells >= 3 else "chain"]
    up = rt.upstream_map(down)
    rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(ncells, 60 + ncells, area, p0, volr0, wh0, wt0, nsub, dt)
    ftab = rt.inundation_tables(area, p, rdepth, eprof) if flood else None
    bytes0 = D.device_bytes
    _enable(D, down, ddist, area, p, nsub, (cap, target, beta, mstart), rows, (rdepth, eprof) if flood else None)
    assert bits(D.routing_read(rt.CMD_RATIO)) == bits(np.ones(ncells)) and not any(D.routing_read(w).any() for w in CMD_ROWS[:3])
    D.routing_init(volr)
    D.routing_kinematic_init(wh, wt)
    if flood:
        D.routing_inundation_init(wf)
    D.routing_reservoir_init(res0, krls0)
    census = [] if ncells == 1001 else None
    crow = _chain(D, rc.NCALLS, (wh, wt, volr, wf, res0, krls0), tab, cmd, hosts, area, p, up, dt, nsub, ftab, census)
    if ncells == 1:
        assert not cmd["HAS"].any() and not any(x.any() for x in crow[:3]) and bits(crow[3]) == bits(np.ones(1))
    else:
        assert (crow[1] > 0.0).any() and (crow[2] > 0.0).any()
    if census is not None:
        assert rc.dam_cells(ncells).size == 143 and cmd["dams"].size > 2 * cc.CMD_DAMS  # (and the dams of the reservoirs' edge values)
        for c, held in enumerate(census):
            assert all(held[k] > 0 for k in cc.CENSUS), (c, held)
    D.routing_clear()  # frees everything
    assert D.device_bytes == bytes0
    D.close()


def test_one_dam_with_2100_dependents(base):
    """2300 cells, one dam in cell 1150 and 2100 cells that hang on it: the dam's span is longer than two tiles of k_command_allot
    (CMD_TILE = 1024), so its sum is carried over three tile passes.  Three calls of two sub-steps against the restatement on every
    row; the dam starts 4e5 m3 above SMIN, is limited, and its ratio lies strictly between 0 and 1."""
    n, nsub, dt = 2300, 2, 1800.0
    D = _ctx(base, None, n)
    ddist, area, p, volr, wh, wt = ic.cell_values(n, 40 + n)
    (cap, target, beta, mstart, res0, krls0), rows = cc.single_dam(n)
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    cmd = rt.command_tables(cap, *rows)
    assert cmd["dams"].tolist() == [1150] and int(cmd["ptr"][1]) == 2100 > 2 * cc.CMD_TILE
    hosts = [host_inputs(D, set_runoff(D, ic.snwcp(c)), area) for c in range(3)]
    down = ic.networks(n, 52 + n)["forest"]
    _enable(D, down, ddist, area, p, nsub, (cap, target, beta, mstart), rows)
    D.routing_init(volr)
    D.routing_kinematic_init(wh, wt)
    D.routing_reservoir_init(res0, krls0)
    crow = _chain(D, 3, (wh, wt, volr, None, res0, krls0), tab, cmd, hosts, area, p, rt.upstream_map(down), dt, nsub)
    assert 0.0 < crow[3][1150] < 1.0 and crow[2][1150] > 0.0
    D.close()


# ---- the edge values ---------------------------------------------------------------------------------------------------------------------
def test_the_edge_values_do_what_the_statement_says(base):
    """One call of one sub-step on a network of outlets (command_cases.edge_values), against the restatement bit for bit and by kind, as
    C8 lists them: NaN, +-inf, negative and tiny RES, RES <= SMIN, a WANT of +inf, W = 0 with terms, a cell whose QIN is NaN."""
    n, dt = 257, 1800.0
    D = rv.context(base, None, n, seed=12, cell_map=ic.cell_map, withdraw=True)
    rate = np.random.default_rng(5).uniform(1.0e-6, 3.0e-5, rc.NCOLS)
    rate[5], rate[9] = 1.7e308, 0.0  # (times the smallest weight and area still an infinite volume; elmk_irrigation_init takes no NaN)
    D.irrigation_init(rate, np.full(rc.NCOLS, 1000.0))
    D.irrigation(DT, 0)
    D._qirr = D.irrigation_read(ir.QFLX_IRRIG)
    assert D._qirr[5] == 1.7e308 and D._qirr[9] == 0.0
    ddist, area, p, volr0, wh0, wt0 = ic.cell_values(n, 40 + n)
    volr0, wh0, wt0 = finite(volr0), finite(wh0), finite(wt0)
    (cap, target, beta, mstart, res0, krls0), rows = cc.edge_values(n)
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    cmd = rt.command_tables(cap, *rows)
    hosts = [host_inputs(D, set_runoff(D, ic.snwcp(0)), area)] * 3
    down = ic.networks(n, 1)["outlets"]
    _enable(D, down, ddist, area, p, 1, (cap, target, beta, mstart), rows)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_reservoir_init(res0, krls0)
    want, take, give, ratio = _chain(D, 1, (wh0, wt0, volr0, None, res0, krls0), tab, cmd, hosts, area, p, rt.upstream_map(down), dt, 1)
    res, qin = D.routing_read(rt.RES), D.routing_read(rt.QIN)
    at = {v if v == v else "nan": cc.EDGE_DAM0 + 2 * i for i, v in enumerate(rc.SPECIAL)}
    deps = np.array(sorted(at.values())) + 1
    assert (want[deps] > 0.0).all() and np.isfinite(want[deps]).all()
    for v in (0.0, -0.0, -3.5e4, 5e-324, "nan", -INF):  # RES <= SMIN, negative, NaN: avail = 0.0, ratio 0.0, nothing is given
        d = at[v]
        assert ratio[d] == 0.0 and give[d] == 0.0 and take[d + 1] == 0.0, v
    assert np.isnan(res[at["nan"]]) and res[at[-INF]] == -INF
    d = at[INF]  # (the K1 launch's regulation comes first: +inf spills down to CAP) gives everything asked
    assert ratio[d] == 1.0 and give[d] == want[d + 1] and take[d + 1] == want[d + 1]
    d = at[1e300]
    assert ratio[d] == 1.0 and give[d] == want[d + 1]
    # WANT = +inf in one term: W = +inf, ratio 0.0, G = NaN - the dam, its GIVE and both dependents' TAKE and QIN
    d = cc.EDGE_INF_DAM
    assert want[cc.EDGE_INF_CELL] == INF and np.isfinite(want[cc.EDGE_INF_PEER]) and want[cc.EDGE_INF_PEER] > 0.0
    assert ratio[d] == 0.0 and np.isnan(give[d]) and np.isnan(res[d])
    assert np.isnan(take[cc.EDGE_INF_CELL]) and np.isnan(qin[cc.EDGE_INF_CELL]) and take[cc.EDGE_INF_PEER] == 0.0
    # W = 0 with terms - two idle cells, one of NaN runoff: ratio 1.0, nothing given, QIN NaN as without the part
    d = cc.EDGE_ZERO_DAM
    assert want[0] == 0.0 and want[cc.EDGE_NAN_CELL] == 0.0 and ratio[d] == 1.0 and give[d] == 0.0 and np.isfinite(res[d])
    assert take[cc.EDGE_NAN_CELL] == 0.0 and np.isnan(qin[cc.EDGE_NAN_CELL])
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING
FLAGS_IRR = FLAGS | st.RUN_IRRIGATION


@pytest.fixture(scope="module")
def run_base():
    """river_cases.run_case with the dams, on a map in which every column lies in at most one cell (the supply limit needs it), with an
    irrigation that applies a rate on every other column - windows that reach their check during a run - and ring_values' rows."""
    G = rv.run_case(dam=True)
    rng = np.random.default_rng(91)
    cnt = rng.integers(0, 4, NCELL)
    while cnt.sum() > NCOL - 3:
        cnt[cnt.argmax()] -= 1
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    G["map"] = (ptr, rng.permutation(NCOL)[:int(ptr[-1])].astype(np.int32), rng.uniform(0.1, 1.0, int(ptr[-1])))
    c = np.arange(NCOL)
    G["sched"] = np.full(NCOL, ir.NOT_IRRIGATED, np.int32)
    G["irr"] = (np.where(c % 2 == 0, 2.0e-5 + 1.0e-7 * (c % 97), 0.0), 8.0 + (c % 6).astype(np.float64))
    G["cmd"] = cc.ring_values(G["dam"][0], claims=(0.1, 0.05))
    assert rt.command_tables(G["dam"][0], *G["cmd"])["HAS"].all()
    return G


def _run_context(G, graph, lib_path=None, init=True, command=True, limit=False, parts=("routing", "kinematic", "inundation", "reservoir")):
    D = rv.run_context(G, graph, lib_path, parts=parts, init=init)
    D.irrigation_enable(G["sched"])
    D.routing_set_withdrawal(True)
    if init:
        _irrigate(D, G)
    if limit:
        D.irrigation_supply_enable(0.1)
    if command:
        D.routing_command_enable(*G["cmd"])
    return D


def _irrigate(D, G):
    """RATE and NLEFT from the case and one stand-alone step, so that QFLX_IRRIG holds the rate."""
    D.irrigation_init(*G["irr"])
    D.irrigation(DT, 0)


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise_and_the_key_follows_the_switches(run_base, graph):
    """elmk_run with the routing and irrigation flags against the stepwise calls in every field and row: with the part on; cleared
    between two runs (the captured step is dropped and the form without it runs); on again with the supply limit, whose launch takes
    the CMD form; the limit cleared; and the part changes what a run computes."""
    steps = rc_month_schedule(2 * NSTEPS)
    rows = rows_of(True)
    A, B = _run_context(run_base, False), _run_context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:3], FLAGS_IRR, reservoir_time=True)
    B.run(DT, steps[:3], FLAGS_IRR)
    a = river_snapshot(A, rows)
    assert_same(river_snapshot(B, rows), a)
    assert (a["route"][len(rows) - 3] > 0.0).any()  # CMD_TAKE
    P = _run_context(run_base, False, command=False)
    P.run(DT, steps[:3], FLAGS_IRR)
    assert bits(P.routing_read(rt.RES)) != bits(a["route"][10]) and bits(P.routing_read(rt.WT)) != bits(a["route"][5])
    P.close()
    stepwise(A, run_base["rec"], steps[3:5], FLAGS_IRR, reservoir_time=True)  # a second run: on the captured step
    B.run(DT, steps[3:5], FLAGS_IRR)
    assert_same(river_snapshot(B, rows), river_snapshot(A, rows))
    for X in (A, B):
        X.routing_command_clear()
    stepwise(A, run_base["rec"], steps[5:7], FLAGS_IRR, reservoir_time=True)
    B.run(DT, steps[5:7], FLAGS_IRR)
    assert_same(river_snapshot(B, rows[:13]), river_snapshot(A, rows[:13]))
    for X in (A, B):
        X.irrigation_supply_enable(0.1)
        X.routing_command_enable(*run_base["cmd"])  # (the limit first, then the part)
    stepwise(A, run_base["rec"], steps[7:10], FLAGS_IRR, reservoir_time=True)
    B.run(DT, steps[7:10], FLAGS_IRR)
    a = river_snapshot(A, rows)
    assert_same(river_snapshot(B, rows), a)
    assert bits(A.irrigation_supply_read(ir.RATIO)) == bits(B.irrigation_supply_read(ir.RATIO))
    for X in (A, B):
        X.irrigation_supply_clear()
    stepwise(A, run_base["rec"], steps[10:], FLAGS_IRR, reservoir_time=True)
    B.run(DT, steps[10:], FLAGS_IRR)
    assert_same(river_snapshot(B, rows), river_snapshot(A, rows))
    for X in (A, B):
        X.close()


def rc_month_schedule(nsteps):
    """run_cases.schedule moved to the end of January: half-hour steps from 22:30 of day 30, so that step 3 starts at 00:00 of
    1 February."""
    S = schedule(nsteps)
    for s in range(nsteps):
        ddoy = 30.9375 + s * DT / 86400.0
        S[s]["decday"], S[s]["doy"] = ddoy + 1.0, int(ddoy)
    return S


# ---- 3. restart ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_restart_3_plus_3_equals_6(run_base, lib_path):
    """Three steps, the column image and beside it the routing's prognostic rows through elmk_routing_read; a fresh context, restart_load
    and the _init calls, three more steps: the bits of six steps in one context on all seventeen rows.  The part has no prognostic
    row: the image is the one a context without it saves, to the byte count."""
    steps = rc_month_schedule(NSTEPS)
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
    _irrigate(Cx, run_base)
    Cx.routing_init(volr, qsum, count)
    Cx.routing_kinematic_init(wh, wt)
    Cx.routing_inundation_init(wf)
    Cx.routing_reservoir_init(res, krls)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, rows), want)
    N = _run_context(run_base, True, lib_path, command=False)
    assert N.restart_size() == size_a
    N.close()
    Cx.close()


def test_restart_3_plus_3_through_a_version_7_image(run_base):
    """Under ELMK_OPT_RESTART_CELLS a context with the part on saves version 7 with the cell sections it had before - no CMD row is in
    the image - and 3 + 3 steps through the image give the bits of 6.  With rows that fill no slot the image is byte for byte the one
    of a context that never had the part."""
    from elmkernels_amd import restart as R
    steps = rc_month_schedule(NSTEPS)
    rows = rows_of(True)
    A = _run_context(run_base, True)
    A.run(DT, steps, FLAGS)
    want = river_snapshot(A, rows)
    A.close()
    B = _run_context(run_base, True)
    B.set_option(st.OPT_RESTART_CELLS, 1)
    B.run(DT, steps[:3], FLAGS)
    img = B.restart_save()
    head = np.frombuffer(img[:R.HEADER.itemsize].tobytes(), R.HEADER)[0]
    assert int(head["version"]) == R.VERSION_RESERVOIR == 7
    off = R.HEADER.itemsize + 16 + int(head["nentries"]) * R.ENTRY.itemsize
    table = np.frombuffer(img[off:off + int(head["nsections"]) * R.SECTION.itemsize].tobytes(), R.SECTION)
    cells = table[table["kind"] == R.ROUTING_SECTION]
    assert cells["id"].tolist() == [rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF, rt.RES, rt.KRLS]
    B.close()
    Cx = _run_context(run_base, True, init=False)
    Cx.set_option(st.OPT_RESTART_CELLS, 1)
    Cx.restart_load(img)
    _irrigate(Cx, run_base)
    assert Cx.routing_count() == 3 and not any(Cx.routing_read(w).any() for w in CMD_ROWS[:3]) and bits(Cx.routing_read(rt.CMD_RATIO)) == bits(np.ones(NCELL))
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(river_snapshot(Cx, rows), want)
    Cx.close()
    empty = (np.full((4, NCELL), -1, np.int32), np.zeros((4, NCELL)), np.zeros((4, NCELL)))
    images = []
    for command in (True, False):
        X = _run_context(run_base, True, command=False)
        X.set_option(st.OPT_RESTART_CELLS, 1)
        if command:
            X.routing_command_enable(*empty)
        X.run(DT, steps[:3], FLAGS)
        images.append(X.restart_save())
        X.close()
    assert images[0].tobytes() == images[1].tobytes()


# ---- 4. the clear and the refusals ---------------------------------------------------------------------------------------------------------
def test_clear_gives_the_bits_of_a_context_that_never_had_the_part(run_base):
    """Two calls with the part, the clear, two calls without: on every other row the bits of a context that never had it, given the same
    storages and RES; the allocation is what it was before the enable, and the rows are out of range."""
    rows = rows_of(True, command=False)
    A = _run_context(run_base, False, command=False)
    B = _run_context(run_base, False, command=False)
    bytes1 = A.device_bytes
    A.routing_command_enable(*run_base["cmd"])
    assert A.device_bytes - bytes1 >= (4 + 8 + 1) * 8 * 128 + 4 * 4 * 128
    for c in range(2):
        set_runoff(A, ic.snwcp(c)[:NCOL])
        A.routing_reservoir_time(c, False)
        A.routing(DT)
    assert (A.routing_read(rt.CMD_TAKE) > 0.0).any()
    held = read_rows(A, rows)
    A.routing_command_clear()
    A.routing_command_clear()  # nothing to free: OK
    assert A.device_bytes == bytes1 == B.device_bytes and A.routing_count() == 2
    for g, h in zip(read_rows(A, rows), held):
        assert bits(g) == bits(h)
    for w in CMD_ROWS:
        with pytest.raises(L.ElmkError, match="unknown row"):
            A.routing_read(w)
    B.routing_init(held[0], held[3], 2)
    B.routing_kinematic_init(held[4], held[5])
    B.routing_inundation_init(held[7])
    B.routing_reservoir_init(held[10], held[11])
    for c in range(2):
        for D in (A, B):
            set_runoff(D, ic.snwcp(c)[:NCOL])
            D.routing_reservoir_time(2, False)
            D.routing(DT)
    for g, h, which in zip(read_rows(A, rows), read_rows(B, rows), rows):
        assert bits(g) == bits(h), NAMES[which]
    A.routing_command_enable(*run_base["cmd"])  # ... and on again: zero-filled, RATIO 1.0
    assert not any(A.routing_read(w).any() for w in CMD_ROWS[:3]) and bits(A.routing_read(rt.CMD_RATIO)) == bits(np.ones(NCELL))
    A.routing_clear()  # frees everything
    A.close()
    B.close()


def test_refusals_change_nothing(run_base):
    """Every refusal of the three entries and of the interlocks, with nothing changed by any."""
    G = run_base
    cap = G["dam"][0]
    dam, share, claim = G["cmd"]

    def refused(*calls, match=None):
        for call in calls:
            with pytest.raises(L.ElmkError, match=match):
                call()

    enable = lambda d=dam, s=share, q=claim: D.routing_command_enable(d, s, q)  # noqa: E731
    D = rv.run_context(G, True, parts=("routing",))
    bytes0 = D.device_bytes
    refused(enable, D.routing_command_budget, match="the scheme is not on")
    D.routing_command_clear()  # nothing to free: OK
    D.routing_kinematic_enable(G["p"])
    D.routing_kinematic_init(G["wh"], G["wt"])
    refused(enable, D.routing_command_budget, match="the extension is not on")
    D.routing_reservoir_enable(*G["dam"][:4])
    D.routing_reservoir_init(*G["dam"][4:])
    refused(enable, match="the routing's withdrawal is not on")
    refused(D.routing_command_budget, match="the command areas are not on")
    refused(*(lambda w=w: D.routing_read(w) for w in CMD_ROWS), lambda: D.routing_read(25), match="unknown row")
    refused(lambda: D.cell_history_add_row(0, st.CELL_ROWS_ROUTING, rt.CMD_TAKE, st.HIST_AVG), match="row out of range")
    D.irrigation_enable(G["sched"])
    D.routing_set_withdrawal(True)
    _irrigate(D, G)
    bytes1, size1 = D.device_bytes, D.restart_size()
    state1 = river_snapshot(D, rows_of(False, command=False))
    free = int(np.nonzero(cap == 0.0)[0][5])
    a_dam = int(dam[0, free])
    bad = [("dam", 0, free, NCELL, rt.E_CMD_RANGE, free), ("dam", 0, free, -2, rt.E_CMD_RANGE, free), ("dam", 0, free, free + 1 if cap[free + 1] == 0.0 else free - 1, rt.E_CMD_NODAM, free),
           ("dam", 3, free, a_dam, rt.E_CMD_GAP, free), ("dam", 0, a_dam, a_dam, rt.E_CMD_SELF, a_dam), ("dam", 1, free, a_dam, rt.E_CMD_TWICE, free),
           ("share", 0, free, 0.0, rt.E_CMD_SHARE, free), ("share", 0, free, NAN, rt.E_CMD_SHARE, free), ("share", 0, free, 1.5, rt.E_CMD_SHARE, free),
           ("claim", 0, free, -0.1, rt.E_CMD_CLAIM, free), ("claim", 0, free, NAN, rt.E_CMD_CLAIM, free),
           ("share", 0, 0, 0.9, rt.E_CMD_SHARE_SUM, 0), ("claim", 0, free, 0.95, rt.E_CMD_CLAIM_SUM, a_dam)]
    for row, k, c, v, text, cell in bad:
        d, s, q = dam.copy(), share.copy(), claim.copy()
        if row == "dam" and k == 1:
            s[1, c], q[1, c] = 0.1, 0.0
        {"dam": d, "share": s, "claim": q}[row][k, c] = v
        with pytest.raises(ValueError) as e:
            rt.check_command(cap, d, s, q)
        assert str(e.value) == rt.e_cell(text, cell), (row, k, c, v)
        refused(lambda d=d, s=s, q=q: enable(d, s, q), match="elmk_routing_command_enable: " + re.escape(rt.e_cell(text, cell)) + "$")
    arrs = [np.ascontiguousarray(dam, dtype=np.int32), np.ascontiguousarray(share), np.ascontiguousarray(claim)]
    ptrs = [x.ctypes.data_as(C.c_void_p) for x in arrs]
    for k in range(3):
        args = list(ptrs)
        args[k] = None
        assert D.lib.elmk_routing_command_enable(D.ctx, *args) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap_:
        rc_ = D.lib.elmk_routing_command_enable(D.ctx, *ptrs)
        cap_.end()
        assert rc_ == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    for call in (lambda: enable(d=dam[:, :-1]), lambda: enable(s=share[:-1]), lambda: enable(q=claim[:, :-1])):
        with pytest.raises(ValueError):
            call()
    assert D.device_bytes == bytes1 and D.restart_size() == size1
    assert_same(river_snapshot(D, rows_of(False, command=False)), state1)

    enable()
    bytes2 = D.device_bytes
    assert bytes2 > bytes1 and D.restart_size() == size1  # the image is what it was
    rows = rows_of(False)
    state2 = river_snapshot(D, rows)
    refused(enable, match="already on")
    refused(D.routing_reservoir_clear, lambda: D.routing_set_withdrawal(False), match="elmk_routing_command_clear first")
    refused(D.routing_kinematic_clear, match="elmk_routing_reservoir_clear first")
    refused(lambda: D.routing_read(25), lambda: D.routing_read(rt.CMD_GIVE, cell0=NCELL, n=1))
    assert D.lib.elmk_routing_command_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap_:
        rcs = (D.lib.elmk_routing_command_clear(D.ctx), D.lib.elmk_routing_command_budget(D.ctx, ptrs[1]))
        cap_.end()
        assert rcs == (-1, -1) and b"captured" in D.lib.elmk_last_error(D.ctx)
    e = D.cell_history_add_row(0, "routing", rt.CMD_GIVE, st.HIST_AVG)
    refused(D.routing_command_clear, match="elmk_history_clear first")
    D.history_clear()
    assert e >= 0 and D.device_bytes == bytes2 and D.restart_size() == size1
    assert_same(river_snapshot(D, rows), state2)
    # the supply limit comes and goes in either order relative to the part
    D.irrigation_supply_enable(0.1)
    D.routing_command_clear()
    D.routing_command_enable(dam, share, claim)
    D.irrigation_supply_clear()
    assert D.device_bytes == bytes2
    # the following call is the call of a context that met no refusal
    W = _run_context(G, True, parts=("routing", "kinematic", "reservoir"))
    for X in (D, W):
        set_runoff(X, ic.snwcp(0)[:NCOL])
        X.routing_reservoir_time(7, True)
        X.routing(DT)
    for g, h, which in zip(read_rows(D, rows), read_rows(W, rows), rows):
        assert bits(g) == bits(h), NAMES[which]
    D.routing_command_clear()
    assert D.device_bytes == bytes1
    enable()
    D.routing_clear()  # frees everything
    assert D.device_bytes < bytes0
    D.close()
    W.close()


# ---- 5. the budget and the supply limit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncells", [2, 65, 1001])
def test_budget_equals_the_restatement(base, ncells):
    D = _ctx(base, None, ncells)
    ddist, area, p, volr0, wh0, wt0 = ic.cell_values(ncells, 40 + ncells)
    volr0, wh0, wt0 = (finite(x) for x in (volr0, wh0, wt0))
    cap, target, beta, mstart, res0, krls0 = cc.reservoir_values(ncells, 90 + ncells)
    res0 = finite(res0)
    q = ic.snwcp(1)
    q[9] = 2.0e-5
    wd = host_inputs(D, set_runoff(D, q), area)[2]
    with np.errstate(all="ignore"):
        rows_in = cc.command_values(ncells, 3, wd[1] > 0.0)
    down = ic.networks(ncells, 5)["forest" if ncells >= 3 else "chain"]
    _enable(D, down, ddist, area, p, 2, (cap, target, beta, mstart), rows_in)
    D.routing_init(volr0)
    D.routing_kinematic_init(wh0, wt0)
    D.routing_reservoir_init(res0, krls0)
    for _ in range(2):
        D.routing(1800.0)
    rows = read_rows(D, rows_of(False))
    give, take = rows[12], rows[11]
    want, want_dam = rt.command_budget(give, take), rt.reservoir_budget(rows[7], rows[9])
    assert np.isfinite(want).all() and (want > 0.0).all() and abs(want[0] - want[1]) <= 1.0e-9 * want[0]
    for _ in range(2):  # (in turn: the budgets share the reduction's scratch)
        assert bits(D.routing_command_budget()) == bits(want)
        assert bits(D.routing_reservoir_budget()) == bits(want_dam)
    for g, h in zip(read_rows(D, rows_of(False)), rows):
        assert bits(g) == bits(h)  # (the calls change no row)
    D.close()


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_the_supply_limit_counts_the_claims(lib_path):
    """C6 (k_irrigation_supply's CMD form) on the shapes of the limit's own device test with the reservoirs: 5003 columns over 70 cells,
    cell 3 with 2100 columns, dams in every third cell and the placed ones, and every cell hanging on the next dam behind it, every
    fourth on the one after that too (command_cases.ring_values).  Ten steps of the seven wrappers and elmk_irrigation with the limit
    behind it; VOLR and RES are set before every step, RES with its own edge values and a third of the dams at or below SMIN: RATE and
    the four cell rows against irrigation.step followed by irrigation.supply_limit(dam=, command=), bit for bit, and not what the DAM
    form alone gives.  After elmk_routing_command_clear the next step is D7's again."""
    n, ncells, thr = 5003, 70, 0.1
    cols, scal, soil, sched = generated(n, 900)
    rows0 = prepare(cols, 614)
    m = sc.cell_map(n, ncells, 51, big=(3, 2100), empty=(0, 61, 62, 63, 64, 65, 66), single=(5, 7), free=50)
    ptr, col, w = m
    area, _ = sc.cell_values(ncells, 52)
    cap, target, beta, mstart = rc.supply_dams(ncells, 54, placed=(0, 3, 5, 8, 9, 10, 11, 12, 13))
    tab = rt.reservoir_tables(cap, target, beta, mstart)
    crow = cc.ring_values(cap)
    cmd = rt.command_tables(cap, *crow)
    D = _new(cols, scal, soil, rows0, lib_path)
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    D.irrigation_enable(sched)
    D.routing_enable(np.full(ncells, -1, np.int32), np.full(ncells, 5.0e4), area, rt.EFFVEL, 1)
    D.routing_set_withdrawal(True)
    D.routing_kinematic_enable(np.repeat(np.array(ic.BASE)[:, None], ncells, axis=1))
    D.routing_reservoir_enable(cap, target, beta, mstart)
    D.routing_command_enable(*crow)
    D.irrigation_supply_enable(thr)
    c = np.arange(n)
    D.irrigation_init(np.where(sched >= 0, 1.0e-4 + 1.0e-6 * (c % 97), 0.0), np.where(c % 3 == 0, (c % 7).astype(np.float64), 0.0))
    smpso = smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    rows, unmet = D.irrigation_rows(), np.zeros(ncells)
    sup_rows = lambda: np.stack([D.irrigation_supply_read(k) for k in (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)])  # noqa: E731
    matters = 0
    for s in range(11):
        tod = (5 * 3600 + 1800 * s) % 86400
        _, volr = sc.cell_values(ncells, 60 + s, lo=2.0 + 0.3 * (s % 6), hi=6.0)
        res = rc.supply_res(cap, 70 + s)
        res[3] = (0.05 + 0.2 * (s % 5)) * cap[3]
        D.routing_init(volr)
        D.routing_reservoir_init(res)
        command = cmd
        if s == 10:
            D.routing_command_clear()
            command = None
        st.timestep7_fused(D, DT)
        fields = {k: D[k] for k in ir.READS}
        _, want = ir.step(fields, rows, sched, DT, tod, smpso, stored=stored)
        args = (ptr, col, w, area, volr, want[ir.RATE], want[ir.NLEFT], int(DT), thr, unmet)
        want_rate, want_sup = ir.supply_limit(*args, qflx_irrig=want[ir.QFLX_IRRIG], dam=(tab, res), command=command)
        plain_rate, plain_sup = ir.supply_limit(*args, qflx_irrig=want[ir.QFLX_IRRIG], dam=(tab, res))
        matters += int(bits(want_sup[ir.RATIO]) != bits(plain_sup[ir.RATIO])) + 100 * int(bits(want_rate) != bits(plain_rate))
        D.irrigation(DT, tod)
        rows, sup = D.irrigation_rows(), sup_rows()
        assert bits(rows[ir.RATE]) == bits(want_rate), (s, "RATE", np.nonzero(rows[ir.RATE] != want_rate)[0][:5])
        assert bits(rows[ir.NLEFT]) == bits(want[ir.NLEFT]) and bits(rows[ir.QFLX_IRRIG]) == bits(want[ir.QFLX_IRRIG]), s
        for k in range(4):
            assert bits(sup[k]) == bits(want_sup[k]), (s, "row", k, np.nonzero(sup[k] != want_sup[k])[0][:5])
        assert bits(D.routing_read(rt.RES)) == bits(res)  # (the limit only reads it)
        unmet = sup[ir.UNMET_SUM]
    assert matters % 100 >= 5 and matters >= 100
    D.close()


# ---- 6. tapes and the example ---------------------------------------------------------------------------------------------------------------
def test_the_rows_on_a_history_tape(run_base):
    """elmk_cell_history_add_row over the four rows while the part is on: the average of three calls is the mean of the rows read after
    each; after the clear the rows are out of range."""
    D = _run_context(run_base, False)
    ids = [D.cell_history_add_row(0, "routing", w, st.HIST_AVG) for w in CMD_ROWS]
    got = []
    for c in range(3):
        set_runoff(D, ic.snwcp(c)[:NCOL])
        D.routing_reservoir_time(c, c == 1)
        D.routing(DT)
        D.history_accumulate()
        got.append(read_rows(D, CMD_ROWS))
    assert (got[-1][1] > 0.0).any()
    for k, e in enumerate(ids):
        acc = -0.0 * np.ones(NCELL)
        for g in got:
            acc = acc + g[k]
        assert bits(D.history_read(e, n=NCELL)) == bits(acc / 3.0), NAMES[CMD_ROWS[k]]
    D.history_clear()
    D.routing_command_clear()
    with pytest.raises(L.ElmkError, match="row out of range"):
        D.cell_history_add_row(0, "routing", rt.CMD_TAKE, st.HIST_AVG)
    D.close()


def test_command_area_demo(tmp_path):
    """examples/command_area_demo.cc builds with g++ against the C ABI and runs: two days with and without the part; with it the crop
    cell's tributary store stays at or above zero and the dam gives what the cell takes; without it the store goes negative."""
    out = run_demo(build_demo("command_area_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(48))
    wt_off, wt_on, take, res = (np.array([float(s[k]) for s in steps]) for k in (1, 2, 3, 4))
    assert wt_off.min() < 0.0 and wt_on.min() >= 0.0 and (take > 0.0).all() and (np.diff(res) < 0.0).all()
    assert sum(s.startswith("command area: ") for s in out) == 1
