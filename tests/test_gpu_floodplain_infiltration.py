"""Floodplain infiltration on the device (include/elmk.h "floodplain infiltration"): k_soil_hydrology's ROF forms, k_water_balance's
LAND forms and k_kinematic_prep's LAND forms against the host restatement (hydrology.step(rof=), water_balance_end(qflx_h2orof_drain=),
routing.kinematic_call(land=)) bit for bit over five chained steps on every map shape, with the frost table, the irrigation's
withdrawal and the reservoirs; the stages inside elmk_run against the stepwise calls, graph on and off, with the extension switched
between runs; the clear; restarts through a version-6 image; the rows on history tapes; every refusal and interlock; the budget."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics
from elmkernels_amd import history as HS
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import floodplain_infiltration_cases as fc
from tests import reservoir_cases as rc
from tests.hydrology_cases import _new, _new_frost
from tests.river_cases import differing, read_rows, river_snapshot
from tests.run_cases import NREC, assert_same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo, same_nan

pytestmark = pytest.mark.gpu

DT, NSUB, TOL, NAN = fc.DT, fc.NSUB, 1.0e-9, float("nan")
ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM, rt.WH, rt.WT, rt.QSUR, rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC)
NAMES = ("VOLR", "QIN", "QOUT", "QOUT_SUM", "WH", "WT", "QSUR", "WF", "FLOOD_DEPTH", "FLOOD_FRAC", "QLAND")
ALL = ROWS + (rt.QLAND,)
DAM_ROWS = (rt.RES, rt.KRLS, rt.RES_TAKE)
WB_FIELDS = hy.WB_READS + ("dtbegin_column_h2o",)
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING
NSTEPS = 6


# ---- contexts ---------------------------------------------------------------------------------------------------------------------------
def _context(G, lib_path=None, irrig=False, dam=None, on=True, run=False, graph=False, upto="all", init=True):
    """A context over the case G with the hydrology (and G's frost rows), the water balance, the output grid, the routing with its
    kinematic-wave scheme and the inundation (upto: "hydrology", "water_balance", "routing", "kinematic" stop earlier), the irrigation
    with the withdrawal (irrig), the reservoirs (dam: reservoir_cases.dam_values' tuple) and (on) the extension."""
    args = (G["cols"], G["scal"], G["soil"], G["rows"])
    geo = (G["lat"], G["lon"]) if "lat" in G else (None, None)
    D = _new_frost(*args, G["frost"], lib_path, *geo) if G["frost"] is not None else _new(*args, lib_path, *geo)
    if run:
        D.set_graph(graph)
        D.run_reserve(NREC, 2 * NSTEPS)
        upload_series(D, G["rec"])
    if upto == "hydrology":
        return D
    D.water_balance_enable(TOL)
    D.set_output_grid(*G["map"], fill=NAN)
    if upto == "water_balance":
        return D
    if irrig:
        n = G["ncols"]
        D.irrigation_enable(np.full(n, ir.NOT_IRRIGATED, np.int32))
        D.irrigation_init(np.where(np.arange(n) % 2 == 0, np.random.default_rng(9).uniform(0.0, 3.0e-5, n), 0.0), np.full(n, 1000.0))
    D.routing_enable(G["down"], G["ddist"], G["area"], rt.EFFVEL, NSUB)
    if irrig:
        D.routing_set_withdrawal(True)
    if init:
        D.routing_init(G["volr"])
    if upto == "routing":
        return D
    D.routing_kinematic_enable(G["p"])
    if init:
        D.routing_kinematic_init(G["wh"], G["wt"])
    if upto == "kinematic":
        return D
    D.routing_inundation_enable(G["rdepth"], G["eprof"])
    if init:
        D.routing_inundation_init(G["wf"])
    if dam is not None:
        D.routing_reservoir_enable(*dam[:4])
        if init:
            D.routing_reservoir_init(fc.finite(dam[4]), dam[5])
    if on:
        D.floodplain_infiltration_enable()
    return D


def _fpi_rows(D):
    return np.stack([D.floodplain_infiltration_read(w) for w in range(hy.FPI_NROWS)])


def _snapshot(D, on=True):
    s = river_snapshot(D, ALL if on else ROWS)
    if on:
        s["fpi"] = _fpi_rows(D)
    return s


def _step(D, irrig=False, time=None):
    """One step through the stand-alone calls, in the run step's order: init_timestep, W0, the irrigation, the soil hydrology, the water
    balance, the routing."""
    st.kokkos_init_timestep(D)
    D.water_balance_begin()
    if irrig:
        D.irrigation(DT, 0)
    D.soil_hydrology(DT)
    D.water_balance(DT, read=False)
    if time is not None:
        D.routing_reservoir_time(*time)
    D.routing(DT)


# ---- 1. the three stages against the restatement ---------------------------------------------------------------------------------------
CHAIN = [pytest.param(shape, None, False, False, False, id=f"{shape}-f64-plain") for shape in fc.SHAPES]
CHAIN += [pytest.param("single", L.F32_LIB_PATH, False, False, False, id="single-f32-plain"),
          pytest.param("single", None, True, False, False, id="single-f64-frost"),
          pytest.param("single", L.F32_LIB_PATH, True, True, False, id="single-f32-frost-irrig"),
          pytest.param("single", None, False, True, False, id="single-f64-irrig"),
          pytest.param("wide", None, True, True, True, id="wide-f64-frost-irrig-dam"),
          pytest.param("single", None, False, False, True, id="single-f64-dam")]


@pytest.mark.parametrize("shape, lib_path, frost, irrig, dam", CHAIN)
def test_five_chained_steps_equal_the_restatement(shape, lib_path, frost, irrig, dam):
    """One routing call without land input (FLOOD_FRAC is zero after elmk_routing_inundation_init, and a<b needs it), then five steps of
    init_timestep, W0, (irrigation,) soil hydrology, water balance, routing.  After every stage of every step what the device holds
    against the restatement on what it held before, bit for bit: the three new column rows, every soil-hydrology row (and frost row),
    h2osoi_liq, h2osoi_ice, h2osoi_vol, h2osfc, every water-balance row, the ten inundation-form cell rows, QLAND (and RES, KRLS,
    RES_TAKE).  The census (floodplain_infiltration_cases.census, on the rows the device held): in the wide shape every branch of F1 -
    a column in no cell, the guard failing on WF, on FLOOD_FRAC, a < b, a >= b - is taken in every step (the guard cannot fail on the
    area first on a device: a cell without area has a FLOOD_FRAC of zero, and the routing refuses a NaN area; the host test of the guard
    meets it); in the other shapes with more than one cell over the chain.  The edge values of WF sit in cells 2, 4 .. 16 (+inf lasts
    until the first routing call turns it into inf - inf, so WF = +inf beyond the guard is the host test's too), the NaN qinmax in a
    column of cell 42, an outlet."""
    G = fc.case(shape, 31, frost=frost)
    dv = rc.dam_values(G["ncells"], 91) if dam else None
    D = _context(G, lib_path, irrig=irrig, dam=dv)
    stored = np.float32 if lib_path else None
    dtab = rt.reservoir_tables(*dv[:4]) if dam else None
    assert not _fpi_rows(D).any() and not D.routing_read(rt.QLAND).any()
    D.floodplain_infiltration_clear()  # (the call that fills FLOOD_FRAC runs the plain forms)
    st.kokkos_init_timestep(D)
    D.water_balance_begin()
    D.upload("qflx_snwcp_liq", np.zeros(G["ncols"]))
    D.water_balance(DT, read=False)
    if dam:
        D.routing_reservoir_time(0, False)
    D.routing(DT)
    D.floodplain_infiltration_enable()
    union = np.zeros(len(fc.BRANCHES), np.int64)
    qsum = D.routing_read(rt.QOUT_SUM)
    for s in range(fc.NSTEPS):
        st.kokkos_init_timestep(D)
        D.water_balance_begin()
        qirr = None
        if irrig:
            D.irrigation(DT, 0)
            qirr = D.irrigation_read(ir.QFLX_IRRIG)
        f = {k: D[k] for k in set(fc.STEP_FIELDS + WB_FIELDS + (("t_soisno",) if frost else ()))}
        rows, wb0 = D.soil_hydrology_rows(), D.water_balance_rows()
        fr = D.soil_hydrology_frost_rows() if frost else None
        cell = read_rows(D, ROWS)
        river = dict(volr=cell[0], wh=cell[4], wt=cell[5], wf=cell[7], frac=cell[9])
        time = None
        if dam:
            time = rc.call_time(s)
            river.update(res=D.routing_read(rt.RES), krls=D.routing_read(rt.KRLS))
        g, rows1, fr1, fpi, wb1, new, qland = fc.host_step(f, rows, wb0, river, G, frost=fr, qirr=qirr, stored=stored,
                                                            dam=dict(tab=dtab, month=time[0], begins=time[1]) if dam else None)
        D.soil_hydrology(DT)
        for k in hy.WRITES:  # (the state fields are stored as formed: the NaN column's NaN has no canonical sign)
            assert same_nan(D[k], g[k]), (s, k)
        assert bits(D.soil_hydrology_rows()) == bits(rows1), (s, "hydrology rows", differing(D.soil_hydrology_rows().reshape(-1), rows1.reshape(-1)))
        if frost:
            assert bits(D.soil_hydrology_frost_rows()) == bits(fr1), (s, "frost rows")
        got = _fpi_rows(D)
        for w, name in enumerate(("H2OROF", "FRAC", "QFLX_H2OROF_DRAIN")):
            assert bits(got[w]) == bits(fpi[w]), (s, name, differing(got[w], fpi[w]))
        D.water_balance(DT, read=False)
        assert bits(D.water_balance_rows()) == bits(wb1), (s, "water balance rows")
        if dam:
            D.routing_reservoir_time(*time)
        D.routing(DT)
        with np.errstate(all="ignore"):
            qsum = rt._canon(qsum + new["qout"])
        want = (new["volr"], new["qin"], new["qout"], qsum, new["wh"], new["wt"], new["qsur"], new["wf"], new["depth"], new["frac"], qland)
        for gr, wr, name in zip(read_rows(D, ALL), want, NAMES):
            assert bits(gr) == bits(wr), (s, name, differing(gr, wr))
        if dam:
            for gr, wr, name in zip(read_rows(D, DAM_ROWS), (new["res"], new["krls"], new["take"]), ("RES", "KRLS", "RES_TAKE")):
                assert bits(gr) == bits(wr), (s, name, differing(gr, wr))
        took = np.bincount(fc.census(G["cellof"], river["wf"], river["frac"], fpi), minlength=len(fc.BRANCHES))
        union += took
        print(f"step {s}: " + ", ".join(f"{b} {t}" for b, t in zip(fc.BRANCHES, took.tolist())))
        if shape == "wide" and not (frost or irrig or dam):
            assert (took > 0).all(), (s, took)
            q = G["nanq"]
            assert fpi[hy.FPI_QFLX_DRAIN, q] == fpi[hy.FPI_H2OROF, q] / DT > 0.0 and np.isnan(rows1[hy.FSAT, q])
        assert not (fpi[hy.FPI_QFLX_DRAIN] < 0.0).any() and not np.isnan(fpi[hy.FPI_QFLX_DRAIN]).any()
        assert (fpi[hy.FPI_QFLX_DRAIN] > 0.0).any() and (qland > 0.0).any()
    if shape != "one":
        assert (union > 0).all(), union
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_base():
    return fc.run_case()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the three flags and the extension on against the stepwise calls in every field and row, then a second
    run (on the captured step when the graph is on); the extension cleared between two runs, which drops the captured step and runs the
    plain forms, and enabled again, which brings the forms back."""
    steps = schedule(2 * NSTEPS)
    A, B = _context(run_base, run=True, graph=False), _context(run_base, run=True, graph=graph)
    stepwise(A, run_base["rec"], steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["fpi"][hy.FPI_QFLX_DRAIN] > 0.0).any() and (a["route"][10] > 0.0).any() and B.routing_count() == NSTEPS
    stepwise(A, run_base["rec"], steps[NSTEPS:], FLAGS)
    B.run(DT, steps[NSTEPS:], FLAGS)
    assert_same(_snapshot(B), _snapshot(A))
    for X in (A, B):
        X.floodplain_infiltration_clear()
    stepwise(A, run_base["rec"], steps[:2], FLAGS)
    B.run(DT, steps[:2], FLAGS)
    assert_same(_snapshot(B, False), _snapshot(A, False))
    for X in (A, B):
        X.floodplain_infiltration_enable()
    stepwise(A, run_base["rec"], steps[2:4], FLAGS)
    B.run(DT, steps[2:4], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["fpi"][hy.FPI_QFLX_DRAIN] > 0.0).any() and B.routing_count() == 2 * NSTEPS + 4
    for X in (A, B):
        X.close()


# ---- 3. the clear ---------------------------------------------------------------------------------------------------------------------------
def test_clear_returns_to_the_stages_without_the_term(run_base):
    """Two steps with the extension, the clear, and a context that never had it given the same columns, hydrology rows and river rows
    (WF among them): two more steps give the same bits in every field and row; the bytes of the extension are returned, and the restart
    image never changed its size."""
    A = _context(run_base)
    B = _context(run_base, on=False)
    bytes_b, size_b = B.device_bytes, B.restart_size()
    assert A.device_bytes - bytes_b >= 8 * A.routing_ncells + 3 * 8 * A.level_stride + 4 * A.level_stride and A.restart_size() == size_b
    for _ in range(2):
        _step(A)
    assert (_fpi_rows(A)[hy.FPI_QFLX_DRAIN] > 0.0).any()
    A.floodplain_infiltration_clear()
    A.floodplain_infiltration_clear()  # nothing to free: OK
    assert A.device_bytes == bytes_b and A.restart_size() == size_b
    with pytest.raises(L.ElmkError, match="unknown row"):
        A.routing_read(rt.QLAND)
    with pytest.raises(L.ElmkError, match="the extension is not on"):
        A.floodplain_infiltration_read(hy.FPI_FRAC)
    for k in A.fields:
        B[k] = A[k]
    hrows = A.soil_hydrology_rows()
    B.soil_hydrology_init(hrows[hy.ZWT], hrows[hy.WA])
    volr, qsum, wh, wt, wf = read_rows(A, (rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF))
    for X in (A, B):  # (the same calls on both: an init zero-fills its part's diagnostics)
        X.routing_init(volr, qsum, 2)
        X.routing_kinematic_init(wh, wt)
        X.routing_inundation_init(wf)
    for _ in range(2):
        _step(A)
        _step(B)
    assert_same(_snapshot(A, False), _snapshot(B, False))
    assert (A.routing_read(rt.WF) > 0.0).any()
    A.close()
    B.close()


# ---- 4. restart -----------------------------------------------------------------------------------------------------------------------------
def test_restart_3_plus_3_through_a_version_6_image(run_base):
    """Under ELMK_OPT_RESTART_CELLS the image of a context with the extension is a version-6 image (WF is in it already; the three
    column rows and QLAND are rewritten by the next step) with one more cell section, FLOOD_FRAC, which F1 reads before the next routing
    call rewrites it: 3 + 3 steps through it give the bits of 6.  A context without the extension saves what it saved, refuses the
    image and is refused by a context with it; with the option off the image is the one it always was."""
    steps = schedule(NSTEPS)
    A = _context(run_base, run=True, graph=True)
    A.run(DT, steps, FLAGS)
    want = _snapshot(A)
    A.close()
    P = _context(run_base, run=True, graph=True, on=False)
    size_off = P.restart_size()
    P.set_option(st.OPT_RESTART_CELLS, 1)
    size_plain = P.restart_size()
    img_plain = P.restart_save()
    B = _context(run_base, run=True, graph=True)
    assert B.restart_size() == size_off  # (the option off: the columns' image, as ever)
    B.set_option(st.OPT_RESTART_CELLS, 1)
    B.run(DT, steps[:3], FLAGS)
    img = B.restart_save()
    info = R.verify(img)
    cells = info["sections"][info["sections"]["kind"] == R.ROUTING_SECTION]
    assert int(info["header"]["version"]) == R.VERSION_ROUTING == 6 and img.size > size_plain
    assert cells["id"].tolist() == [rt.VOLR, rt.QOUT_SUM, rt.WH, rt.WT, rt.WF, rt.FLOOD_FRAC] and (cells["extent"] == run_base["ncells"]).all()
    B.floodplain_infiltration_clear()
    assert B.restart_size() == size_plain
    B.close()
    with pytest.raises(L.ElmkError):
        P.restart_load(img)  # the extension's image into a context without it
    P.close()
    Cx = _context(run_base, run=True, graph=True, init=False)
    Cx.set_option(st.OPT_RESTART_CELLS, 1)
    with pytest.raises(L.ElmkError):
        Cx.restart_load(img_plain)  # ... and the other way round
    Cx.restart_load(img)
    assert Cx.routing_count() == 3
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(_snapshot(Cx), want)
    Cx.close()


# ---- 5. tapes, refusals, interlocks ---------------------------------------------------------------------------------------------------------
def test_rows_on_history_tapes(run_base):
    """A column entry on QFLX_H2OROF_DRAIN (AVG, MAX) and a cell entry on QLAND (AVG) equal the numpy folds of
    the rows read after each step; while they exist elmk_floodplain_infiltration_clear is refused and changes nothing."""
    D = _context(run_base)
    col = {op: D.history_add_row(0, "floodplain", hy.FPI_QFLX_DRAIN, op) for op in ("avg", "max")}
    cell = D.cell_history_add_row(0, "routing", rt.QLAND, "avg")
    drains, qlands = [], []
    for _ in range(3):
        _step(D)
        D.history_accumulate()
        drains.append(_fpi_rows(D)[hy.FPI_QFLX_DRAIN])
        qlands.append(D.routing_read(rt.QLAND))
    assert (np.array(drains) > 0.0).any() and (np.array(qlands) > 0.0).any()
    for op, e in col.items():
        assert bits(D.history_read(e)) == bits(HS.fold_cell_rows(op, drains)), op
    assert bits(D.history_read(cell)) == bits(HS.fold_cell_rows("avg", qlands))
    state, nbytes = _snapshot(D), D.device_bytes
    with pytest.raises(L.ElmkError, match="elmk_history_clear first"):
        D.floodplain_infiltration_clear()
    assert D.device_bytes == nbytes
    assert_same(_snapshot(D), state)
    D.history_clear()
    cell = D.cell_history_add_row(0, "routing", rt.QLAND, "max")
    with pytest.raises(L.ElmkError, match="elmk_history_clear first"):
        D.floodplain_infiltration_clear()
    D.history_clear()
    D.floodplain_infiltration_clear()
    for call in (lambda: D.history_add_row(0, "floodplain", hy.FPI_QFLX_DRAIN, "avg"), lambda: D.cell_history_add_row(0, "routing", rt.QLAND, "avg")):
        with pytest.raises(L.ElmkError):
            call()
    D.close()


def test_refusals_change_nothing(run_base):
    """Each missing prerequisite by name, a shared column named in the text, the capture, a second enable; each interlocked clear and
    the output grid's set and clear while the extension is on; QLAND and the column rows while it is off: ELMK_E_INVALID with every byte
    and row as it was."""
    G = run_base

    def refused(call, match):
        with pytest.raises(L.ElmkError, match=match):
            call()

    for upto, match in (("hydrology", "the water balance is not enabled"), ("water_balance", r"not enabled \(elmk_routing_enable\)"),
                        ("routing", "the scheme is not on"), ("kinematic", r"the extension is not on \(elmk_routing_inundation_enable\)")):
        D = _context(G, upto=upto, on=False)
        nbytes = D.device_bytes
        refused(D.floodplain_infiltration_enable, match)
        refused(D.floodplain_infiltration_budget, "elmk_floodplain_infiltration_budget")
        refused(lambda: D.floodplain_infiltration_read(0), "elmk_floodplain_infiltration_read")
        D.floodplain_infiltration_clear()  # nothing to free: OK
        assert D.device_bytes == nbytes
        D.close()
    from tests import helpers as H
    D = H.device_state(G["cols"], G["scal"], G["soil"], lat=G["lat"], lon=G["lon"])
    refused(D.floodplain_infiltration_enable, "the soil hydrology is not enabled")
    D.close()
    # a column in two cells: the output grid takes the map, the extension names the column
    ptr, col, w = G["map"]
    col2 = col.copy()
    shared = int(col2[3])
    col2[int(ptr[-1]) - 1] = shared
    S = _context(dict(G, map=(ptr, col2, w)), on=False)
    nbytes, state = S.device_bytes, _snapshot(S, False)
    refused(S.floodplain_infiltration_enable, f"elmk_floodplain_infiltration_enable: column {shared} is in more than one cell")
    assert S.device_bytes == nbytes
    assert_same(_snapshot(S, False), state)
    S.close()

    D = _context(G, on=False)
    bytes0, size0, state0 = D.device_bytes, D.restart_size(), _snapshot(D, False)
    refused(lambda: D.routing_read(rt.QLAND), "unknown row")
    refused(lambda: D.cell_history_add_row(0, "routing", rt.QLAND, "avg"), "row out of range")
    refused(lambda: D.floodplain_infiltration_read(hy.FPI_H2OROF), "the extension is not on")
    with captured(D) as cap:
        rc_ = D.lib.elmk_floodplain_infiltration_enable(D.ctx)
        cap.end()
        assert rc_ == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(_snapshot(D, False), state0)
    D.floodplain_infiltration_enable()
    bytes1 = D.device_bytes
    assert bytes1 > bytes0 and D.restart_size() == size0
    _step(D)
    state1 = _snapshot(D)
    refused(D.floodplain_infiltration_enable, "already on")
    for call in (D.routing_inundation_clear, D.soil_hydrology_clear, D.water_balance_clear, D.clear_output_grid,
                 lambda: D.set_output_grid(*G["map"], fill=NAN), D.routing_kinematic_clear):
        refused(call, "elmk_floodplain_infiltration_clear first|elmk_routing_inundation_clear first")
    for call in (D.routing_inundation_clear, D.soil_hydrology_clear, D.water_balance_clear, D.clear_output_grid,
                 lambda: D.set_output_grid(*G["map"], fill=NAN)):
        refused(call, "the floodplain infiltration is on \\(elmk_floodplain_infiltration_clear first\\)")
    refused(lambda: D.routing_heat_enable(0), "first")
    refused(lambda: D.floodplain_infiltration_read(3), "unknown row")
    refused(lambda: D.floodplain_infiltration_read(0, col0=G["ncols"], n=1), "column range")
    assert D.lib.elmk_floodplain_infiltration_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap:
        rcs = (D.lib.elmk_floodplain_infiltration_clear(D.ctx), D.lib.elmk_floodplain_infiltration_budget(D.ctx, None))
        cap.end()
        assert rcs == (-1, -1)
    assert D.device_bytes == bytes1
    assert_same(_snapshot(D), state1)
    # the following step is the step of a context that met no refusal
    W = _context(G)
    _step(W)
    _step(W)
    _step(D)
    assert_same(_snapshot(D), _snapshot(W))
    D.routing_clear()  # frees it with the rest
    refused(lambda: D.floodplain_infiltration_read(0), "not enabled")
    D.soil_hydrology_clear()  # (nothing holds it any more)
    D.close()
    W.close()


# ---- 6. the budget ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["one", "single"])
def test_budget_equals_the_reduction(shape):
    """elmk_floodplain_infiltration_budget against diagnostics.reduce_min_max_sum of the QLAND row, bit for bit, in turn with the other
    parts' budgets (they share the reduction's scratch); the calls change no row."""
    G = fc.case(shape, 31)
    for k in ("wf", "volr", "wh", "wt"):
        G[k] = fc.finite(G[k])
    if G["nanq"] >= 0:
        G["rows"][hy.WTFACT, G["nanq"]] = 0.3
    D = _context(G)
    _step(D)
    _step(D)
    rows = read_rows(D, ALL)
    want = np.array([diagnostics.reduce_min_max_sum(rows[10])[2]])
    assert np.isfinite(want).all() and want[0] > 0.0 and bits(want) == bits(rt.land_budget(rows[10]))
    for _ in range(2):
        assert bits(D.floodplain_infiltration_budget()) == bits(want)
        assert bits(D.routing_inundation_budget()) == bits(rt.inundation_budget(rows[7]))
    for g, h in zip(read_rows(D, ALL), rows):
        assert bits(g) == bits(h)
    D.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------------------
def test_floodplain_infiltration_demo(tmp_path):
    """examples/floodplain_infiltration_demo.cc builds with g++ against the C ABI and runs: 48 steps with and without the extension; the
    land takes water from the floodplains, the coupled columns end wetter than the plain ones and the coupled floodplains hold less."""
    out = run_demo(build_demo("floodplain_infiltration_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(48))
    wf_plain, wf_on, soil_plain, soil_on, took = (np.array([float(s[k]) for s in steps]) for k in (1, 2, 3, 4, 5))
    assert wf_plain.max() > 0.0 and took.max() > 0.0 and (took >= 0.0).all()
    assert (wf_on <= wf_plain).all() and (wf_on < wf_plain).any() and soil_on[-1] > soil_plain[-1]
    assert sum(s.startswith("the land took") for s in out) == 1
