"""elmk_run's step with every optional part on at once (tests/full_step_cases.py): the run against the stand-alone calls in RUN_STEP's
order, graph on and off, in both builds; the walk of test_gpu_run.py's key test continued through every part of the step's
configuration that the captured step is keyed by or dropped for, one change at a time with all the other stages' nodes in the same
graph; and E3SM's exact-restart test over the full case.  Every comparison is bit for bit."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import full_step_cases as fc
from tests.parity_cases import WETLAND
from tests.run_cases import schedule
from tests.support import same

pytestmark = pytest.mark.gpu

F = fc.ALL_FLAGS
LIBS = {"f64": None, "f32": L.F32_LIB_PATH}


# ---- a. every stage on ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stepwise_reference():
    """Per build, computed once: context A stepped through the stand-alone calls, its snapshot after 6 and after 12 steps (the
    diagnostics rows of a snapshot are those of the six steps before it), what it held before the first step, and the two contexts the
    liveness lines compare with - P, never limited, and W, never limited and without the withdrawal - after twelve steps of elmk_run."""
    out = {}

    def get(build):
        if build not in out:
            G = fc.case()
            steps = schedule(fc.NSTEPS)
            A = fc.full_context(False, LIBS[build])
            before = fc.full_snapshot(A)
            fc.full_stepwise(A, G["rec"], steps[:fc.HALF])
            a6 = fc.full_snapshot(A)
            fc.full_stepwise(A, G["rec"], steps[fc.HALF:])
            a12 = fc.full_snapshot(A)
            A.close()
            others = {}
            for name, kw in (("P", dict(thr=None)), ("W", dict(thr=None, withdraw=False))):
                D = fc.full_context(True, LIBS[build], **kw)
                fc.run(D, steps)
                others[name] = fc.full_snapshot(D)
                D.close()
            out[build] = (before, a6, a12, others["P"], others["W"])
        return out[build]

    return get


@pytest.mark.parametrize("build", ["f64", "f32"])
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_every_stage_on_equals_stepwise(stepwise_reference, graph, build):
    """Twelve steps of run_cases.schedule() with all nine flags as two runs of six (with the graph on the second run replays the step
    the first captured) against full_stepwise: after each run full_snapshot is equal.  Then, on the stepwise context's snapshot, every
    stage was live, so that the equality is not an equality of nothing."""
    before, a6, a12, p, w = stepwise_reference(build)
    steps = schedule(fc.NSTEPS)
    B = fc.full_context(graph, LIBS[build])
    fc.run(B, steps[:fc.HALF])
    fc.assert_same_snapshot(fc.full_snapshot(B), a6, "after six steps")
    fc.run(B, steps[fc.HALF:])
    fc.assert_same_snapshot(fc.full_snapshot(B), a12, "after twelve steps")
    B.close()
    G = fc.geometry()
    irr, sup = a12["rows/irrigation"], a12["rows/supply"]
    assert (irr[ir.QFLX_IRRIG] > 0.0).any() and (a6["rows/irrigation"][ir.QFLX_IRRIG] > 0.0).any()
    assert (irr[ir.NLEFT] == 0.0).any() and (G["sched"] >= 0).sum() > (irr[ir.NLEFT] > 0.0).sum() > 0  # windows open in some columns only
    assert (sup[ir.UNMET_SUM] > 0.0).any() and (sup[ir.UNMET_SUM] == 0.0).any()
    # the limit cut rates back: against the context that was never limited no rate is larger and some are smaller
    rate, free = irr[ir.RATE], p["rows/irrigation"][ir.RATE]
    assert p["rows/supply"] is None and (rate <= free).all() and (rate < free).any()
    volr, wf, frac, qout = (a12[f"route/{k}"] for k in (rt.VOLR, rt.WF, rt.FLOOD_FRAC, rt.QOUT))
    assert (wf > 0.0).any() and (frac > 0.0).any() and (wf == 0.0).any() and (frac == 0.0).any() and (qout > 0.0).any()
    hub = G["hub"]
    assert before[f"route/{rt.WF}"][hub] == 0.0 and a6[f"route/{rt.WF}"][hub] > 0.0  # a cell crossed its bank during the run
    assert int(a12["route/count"]) == fc.NSTEPS
    # the withdrawal: between two contexts that were never limited QIN differs exactly through it, and the full context's differs too
    qin, qin_p, qin_w = (x[f"route/{rt.QIN}"] for x in (a12, p, w))
    assert same(p["rows/irrigation"], w["rows/irrigation"]) and not same(qin_p, qin_w) and (qin_p <= qin_w).all() and not same(qin, qin_w)
    assert a12["rows/frost"][hy.FROST_TABLE].any() and a12["rows/frost"][hy.QFLX_DRAIN_PERCHED].any()
    assert all(a12["rows/alt"][k].any() for k in range(3)) and not same(a12["rows/alt"], before["rows/alt"])
    assert a12["rows/hydrology"][hy.QFLX_DRAIN].any() and np.isfinite(a12["rows/water_balance"]).all()
    for s in fc.AEROSOL_STREAMS:  # the deposition moved with the month bracket
        assert a12["aer_" + s].any() and not same(a12["aer_" + s], a6["aer_" + s]) and not same(a6["aer_" + s], before["aer_" + s])
    hist = [v for k, v in a12.items() if k.startswith("hist/")]
    assert len(hist) == len(fc.FIELD_ENTRIES) + 2 * len(fc.ROW_ENTRIES) and all(int(n) == fc.NSTEPS and v is not None for n, v in hist)
    accum = [v for k, v in a12.items() if k.startswith("accum/")]
    assert len(accum) == 2 and all(int(n) == fc.NSTEPS for n, _ in accum)
    assert a12["diag/cons"].shape == (fc.HALF, 8, 3) and a12["diag/wb_triples"].shape == (fc.HALF, 3, 3)


# ---- b. the step follows its configuration ----------------------------------------------------------------------------------------------
WALK_FAMILIES = ("alt", "hydrology", "water_balance")  # (a family with a history entry over its rows cannot be cleared)


def _carry_routing(D):
    D._route = dict(volr=D.routing_read(rt.VOLR), qsum=D.routing_read(rt.QOUT_SUM), count=D.routing_count(), wh=D.routing_read(rt.WH),
                    wt=D.routing_read(rt.WT), wf=D.routing_read(rt.WF))


def _frost_clear(D):
    D.soil_hydrology_frost_clear()


def _frost_enable(D):
    D.soil_hydrology_frost_enable(fc.case()["frost"][hy.Q_PERCH_MAX])


def _supply_clear(D):
    D._unmet = D.irrigation_supply_read(ir.UNMET_SUM)
    D.irrigation_supply_clear()


def _supply_enable(D, carried=True):
    D.irrigation_supply_enable(fc.THR)
    if carried:
        D.irrigation_supply_init(D._unmet)


def _irrigation_clear(D):
    D._irr = D.irrigation_rows()
    D.irrigation_clear()


def _irrigation_enable(D, sched=None):
    D.irrigation_enable(fc.case()["sched"] if sched is None else sched)
    D.irrigation_init(D._irr[ir.RATE], D._irr[ir.NLEFT])


def _inundation_clear(D):
    D._wf = D.routing_read(rt.WF)
    D.routing_inundation_clear()


def _inundation_enable(D):
    G = fc.case()
    D.routing_inundation_enable(G["rdepth"], G["eprof"])
    D.routing_inundation_init(D._wf)


def _kinematic_clear(D):
    D._kw = (D.routing_read(rt.WH), D.routing_read(rt.WT))
    D.routing_kinematic_clear()


def _kinematic_enable(D):
    D.routing_kinematic_enable(fc.case()["params"])
    D.routing_kinematic_init(*D._kw)


def _other_network(which):
    def change(D):
        _supply_clear(D)  # (the limit bars elmk_routing_clear)
        _carry_routing(D)
        D.routing_clear()
        fc.enable_routing(D, fc.case(), which)
        r = D._route
        D.routing_init(r["volr"], r["qsum"], r["count"])
        D.routing_kinematic_init(r["wh"], r["wt"])
        D.routing_inundation_init(r["wf"])
        _supply_enable(D)
    return change


def _new_irrigation_parameters(D):
    """Another sched row: every irrigated column's local clock an hour on.  The parameter is set by elmk_irrigation_enable, so the
    limit and the withdrawal go first and come back, RATE, NLEFT and UNMET_SUM carried through read / init."""
    sched = fc.case()["sched"]
    _supply_clear(D)
    D.routing_set_withdrawal(False)
    _irrigation_clear(D)
    _irrigation_enable(D, np.where(sched >= 0, (sched + 3600) % 86400, -1).astype(np.int32))
    D.routing_set_withdrawal(True)
    _supply_enable(D)


def _wetland(D):
    """Two steps as a wetland leave NaN soil temperatures in these columns, whose state is a soil column's; every field is kept, so
    that the rest of the walk compares numbers."""
    D.snapshot_fields(list(D.fields))
    D.set_land(**WETLAND)


def _soil_again(D):
    D.restore_fields()
    D.snapshot_fields([])
    D.set_land(**D._land0)


def _more_row_entries(D):
    fc.add_row_entries(D, ("frost", "irrigation"), (2, 3))


NO_IRR = F & ~st.RUN_IRRIGATION
WALK_1 = [  # (what changes, the flags from here on, the change, dt)
    ("nothing: the first capture", F, None),
    ("1 frost table cleared (hyd_frost)", F, _frost_clear),
    ("1 frost table enabled again", F, _frost_enable),
    ("2 IRRIGATION flag off, the irrigation still enabled (irr_stage, irr_supply off; wb_irrig stays)", NO_IRR, None),
    ("3 supply limit cleared", NO_IRR, _supply_clear),
    ("3 withdrawal off (route_withdraw)", NO_IRR, lambda D: D.routing_set_withdrawal(False)),
    ("3 irrigation cleared (wb_irrig off)", NO_IRR, _irrigation_clear),
    ("4 irrigation enabled again, the flag still off (wb_irrig on alone)", NO_IRR, _irrigation_enable),
    ("5 IRRIGATION flag on", F, None),
    ("6 withdrawal on (key only)", F, lambda D: D.routing_set_withdrawal(True)),
    ("6 withdrawal off", F, lambda D: D.routing_set_withdrawal(False)),
    ("6 withdrawal on again", F, lambda D: D.routing_set_withdrawal(True)),
    ("7 supply limit on (irr_supply)", F, lambda D: _supply_enable(D, carried=False)),
    ("7 supply limit off", F, _supply_clear),
    ("7 supply limit on again, UNMET_SUM carried", F, _supply_enable),
    ("8 inundation cleared", F, _inundation_clear),
    ("8 inundation enabled again, WF carried", F, _inundation_enable),
    # (a run between the two clears, so that elmk_routing_kinematic_clear meets a captured step and has to drop it itself)
    ("9 inundation cleared first", F, _inundation_clear),
    ("9 kinematic scheme cleared: the linear scheme, nsub odd", F, _kinematic_clear),
    ("9 kinematic scheme enabled again, WH and WT carried", F, _kinematic_enable),
    ("9 inundation enabled again, WF carried", F, _inundation_enable),
]
WALK_2 = [
    ("nothing: the first capture", F, None),
    ("10 routing cleared, enabled with network B (npad 1) and nsub 2", F, _other_network("B")),
    ("10 back to network A (npad 8) and nsub 3", F, _other_network("A")),
    ("11 ROUTING flag off", F & ~st.RUN_ROUTING, None),
    ("11 ROUTING flag on", F, None),
    ("12 WATER_BALANCE, ROUTING and IRRIGATION off together", F & ~(st.RUN_WATER_BALANCE | st.RUN_ROUTING | st.RUN_IRRIGATION), None),
    ("12 ... and on", F, None),
    ("13 land unit wetland (hyd_stage, irr_stage and irr_supply drop out together)", F, _wetland),
    ("13 land unit soil again", F, _soil_again),
    ("14 new irrigation parameters", F, _new_irrigation_parameters),
    ("15 dt 900", F, None, 900.0),
    ("15 dt 1800", F, None),
    ("16 CF_HALF_WORKGROUPS on", F, lambda D: D.set_option(st.OPT_CF_HALF_WORKGROUPS, 1)),
    ("16 CF_HALF_WORKGROUPS off", F, lambda D: D.set_option(st.OPT_CF_HALF_WORKGROUPS, 0)),
    ("17 run_reserve again, the series uploaded again", F, lambda D: fc.reserve(D, fc.case(), 2)),
    ("18 all nine flags, row entries of the two other families on tapes 2 and 3", F, _more_row_entries),
    ("19 flags 0", 0, None),
    ("all nine flags again", F, None),
]


def _walk(items):
    """Two full contexts, one replaying its captured step and one enqueueing stage by stage; per item one change applied to both, a
    two-step run, and full_snapshot compared.  Returns the snapshots of the graph context."""
    sch = schedule(fc.NSTEPS)
    pair = [fc.full_context(graph, families=WALK_FAMILIES) for graph in (True, False)]
    for D in pair:
        D._land0 = dict(D.land)
    shots = []
    for k, item in enumerate(items):
        what, flags, change = item[:3]
        dt = item[3] if len(item) > 3 else fc.DT
        for D in pair:
            if change:
                change(D)
            fc.run(D, sch[2 * (k % 6):2 * (k % 6) + 2], flags, dt)
        a, b = (fc.full_snapshot(D) for D in pair)
        fc.assert_same_snapshot(a, b, what)
        shots.append(a)
    for D in pair:
        D.close()
    return shots


def test_the_step_follows_its_configuration_hydrology_irrigation_routing_switches():
    """Items 1 - 9 of the walk: the frost table, the irrigation's flag, rows, supply limit and withdrawal, the inundation and the
    kinematic scheme, each switched with everything else on.  That a switch is seen at all is asserted where the rows show it: the part
    that was switched off is None in the snapshot, or the rows it feeds moved."""
    shots = _walk(WALK_1)
    names = [w for w, *_ in WALK_1]
    at = lambda text: shots[next(i for i, w in enumerate(names) if w.startswith(text))]  # noqa: E731
    assert at("1 frost table cleared")["rows/frost"] is None and at("1 frost table enabled")["rows/frost"] is not None
    assert at("3 supply")["rows/supply"] is None and at("3 irrigation cleared")["rows/irrigation"] is None
    # with the flag off the rows stand still; the water balance still takes the stale QFLX_IRRIG until the rows are freed
    assert same(at("2 ")["rows/irrigation"], at("3 withdrawal")["rows/irrigation"]) and (at("2 ")["rows/irrigation"][ir.QFLX_IRRIG] > 0.0).any()
    assert at("7 supply limit off")["rows/supply"] is None
    assert (at("7 supply limit on again")["rows/supply"][ir.UNMET_SUM] >= at("7 supply limit on (")["rows/supply"][ir.UNMET_SUM]).all()
    assert at("8 inundation cleared")[f"route/{rt.WF}"] is None and at("8 inundation enabled")[f"route/{rt.WF}"].any()
    assert at("9 kinematic scheme cleared")[f"route/{rt.WH}"] is None and at("9 kinematic scheme enabled")[f"route/{rt.WH}"].any()
    assert at("9 kinematic scheme enabled")[f"route/{rt.WF}"] is None and at("9 inundation enabled")[f"route/{rt.WF}"].any()
    assert int(shots[-1]["route/count"]) == 2 * len(WALK_1)


def test_the_step_follows_its_configuration_networks_flags_land_dt_options():
    """Items 10 - 19 of the walk: another network and nsub, the run flags of the hydrology family singly and together, the land unit,
    new irrigation parameters, dt, the launch option, a new reservation, more history entries, flags 0 and back."""
    shots = _walk(WALK_2)
    names = [w for w, *_ in WALK_2]
    at = lambda text: shots[next(i for i, w in enumerate(names) if w.startswith(text))]  # noqa: E731
    counts = [int(s["route/count"]) for s in shots]
    routed = [bool(item[1] & st.RUN_ROUTING) for item in WALK_2]
    assert counts == list(np.cumsum([2 if r else 0 for r in routed]))
    # on the wetland the hydrology family stands still
    for k in ("rows/hydrology", "rows/irrigation", "rows/supply", "rows/water_balance"):
        assert same(at("13 land unit wetland")[k], at("12 ... and on")[k]), k
        assert not same(at("13 land unit soil")[k], at("12 ... and on")[k]), k
    # tapes 0 and 1 sampled in every run that carried ELMK_RUN_HISTORY; tapes 2 and 3 hold the four new entries and two runs
    counts = sorted(int(v[0]) for k, v in shots[-1].items() if k.startswith("hist/"))
    sampled = 2 * sum(bool(item[1] & st.RUN_HISTORY) for item in WALK_2)
    assert counts == [4] * 4 + [sampled] * (len(fc.FIELD_ENTRIES) + 2 * len(WALK_FAMILIES))


# ---- c. exact restart ------------------------------------------------------------------------------------------------------------------
# Left out of the comparison: nothing.  The rows INTEGRATION.md documents as per-step diagnostics (QIN, QOUT, QSUR, FLOOD_DEPTH,
# FLOOD_FRAC; DEMAND, COMMITTED, RATIO; QFLX_IRRIG; the water balance's and the frost table's rows) are zeroed by the init calls or
# missing from the image, and the six steps after the restart rewrite every one of them.
ERS_SKIP = ()


@pytest.mark.parametrize("build", ["f64"])
def test_ers_with_every_stage_on(build):
    """E3SM's exact-restart test over the full case: twelve steps in one context against six steps, elmk_restart_save and beside it
    the documented side reads (VOLR, QOUT_SUM and the count; WH and WT; WF; UNMET_SUM), a fresh full context whose every field outside
    the image is poisoned and whose rows were never initialised, elmk_restart_load and the matching init calls, and six more steps."""
    steps = schedule(fc.NSTEPS)
    A = fc.full_context(True, LIBS[build])
    fc.run(A, steps[:fc.HALF])
    fc.run(A, steps[fc.HALF:])
    want = fc.full_snapshot(A)
    A.close()
    B = fc.full_context(True, LIBS[build])
    fc.run(B, steps[:fc.HALF])
    img = B.restart_save()
    _carry_routing(B)
    side, unmet = B._route, B.irrigation_supply_read(ir.UNMET_SUM)
    assert side["count"] == fc.HALF and (side["wf"] > 0.0).any() and (unmet > 0.0).any() and (B.irrigation_read(ir.NLEFT) > 0.0).any()
    B.close()
    Cx = fc.full_context(True, LIBS[build], init=False, poisoned=True)
    Cx.restart_load(img)
    Cx.routing_init(side["volr"], side["qsum"], side["count"])
    Cx.routing_kinematic_init(side["wh"], side["wt"])
    Cx.routing_inundation_init(side["wf"])
    Cx.irrigation_supply_init(unmet)
    fc.run(Cx, steps[fc.HALF:])
    fc.assert_same_snapshot(fc.full_snapshot(Cx), want, "6 + 6 against 12", skip=ERS_SKIP)
    Cx.close()
