"""The full-step case (tests/full_step_cases.py) is not vacuous: conditions on its inputs, computed from the host restatements alone
(irrigation.time_of_day / seconds_since_start / supply_limit, routing.check_network / upstream_map / npad_of / inundation_tables /
kinematic_call, and the path census of tests/inundation_cases.py), before anyone spends a GPU run on it.  They hold by construction."""
import numpy as np

from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from tests import full_step_cases as fc
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc


def _schedule():
    """run_cases.schedule()'s (decday, doy) of the twelve steps: half-hour steps from 21:00 of day 13 (kept apart from run_cases,
    which needs the library's field table)."""
    ddoy = 13.875 + np.arange(fc.NSTEPS) * fc.DT / 86400.0
    return [(float(d + 1.0), int(d)) for d in ddoy]


def test_the_schedule_is_run_cases_schedule():
    from tests.run_cases import schedule

    S = schedule(fc.NSTEPS)
    assert [(float(p["decday"]), int(p["doy"])) for p in S] == _schedule()
    assert [int(p["forc_slot"]) for p in S] == [s // 2 for s in range(fc.NSTEPS)] and max(int(p["forc_slot"]) for p in S) + 1 < fc.NREC
    tods = [ir.time_of_day(d, y) for d, y in _schedule()]
    assert tods[0] == 75600 and 0 in tods  # from 21:00 across midnight
    assert {(int(p["month1"]), int(p["month2"])) for p in S} == {(11, 0), (0, 1)}  # the month bracket moves


def test_both_networks_are_legal_and_pad_to_8_and_1():
    G = fc.geometry()
    for which, npad in (("A", 8), ("B", 1)):
        down, nsub = fc.network(G, which)
        rt.check_network(down, G["ddist"], G["area"])  # raises on a refusal of elmk_routing_enable
        up = rt.upstream_map(down)
        assert rt.npad_of(up) == npad and down.size == fc.NCELL
    up = rt.upstream_map(G["down_a"])
    srcs = up[:, G["hub"]]
    assert (srcs >= 0).all() and (srcs < G["hub"]).sum() == 4 and (srcs > G["hub"]).sum() == 4  # upstream cells on both sides
    assert sorted(srcs.tolist()) == G["srcs"].tolist()
    assert sorted({int(x) for x in (rt.upstream_map(G["down_a"]) >= 0).sum(axis=0)})[-1] == 8
    assert (fc.NCELL + 63) // 64 * 64 == 128 and fc.NCELL - 64 == 6  # a second 64-block that holds six cells


def test_both_nsub_parities_are_present():
    assert fc.NSUB_A % 2 == 1 and fc.NSUB_B % 2 == 0 and fc.network(fc.geometry(), "A")[1] == fc.NSUB_A


def test_the_map_keeps_the_supply_cases_shapes():
    ptr, col, w = fc.geometry()["map"]
    cnt = np.diff(ptr)
    assert ptr.size == fc.NCELL + 1 and (cnt[[0, 63, 64]] == 0).all() and cnt[5] == 1
    assert np.unique(col).size == col.size == fc.NCOL - 3  # every column in at most one cell, three in none
    assert fc.NCOL % 64 != 0 and fc.NCOL < 256


def test_some_columns_pass_their_time_of_day_and_some_never_do():
    G = fc.geometry()
    sched = G["sched"]
    idt = int(fc.DT)
    passes = np.zeros((fc.NSTEPS, fc.NCOL), bool)
    for s, (decday, doy) in enumerate(_schedule()):
        passes[s] = (sched >= 0) & (ir.seconds_since_start(np.maximum(sched, 0), ir.time_of_day(decday, doy)) < idt)
    once = passes.sum(axis=0)
    assert once.max() == 1  # a column checks at most once in the twelve steps
    assert passes.any(axis=1).all()  # some column checks in every step, the step that starts at midnight among them
    never = (sched >= 0) & (once == 0)
    assert (once == 1).sum() > 100 and never.sum() > 20 and (sched < 0).sum() > 20
    c = np.arange(fc.NCOL)
    assert (c[never] % fc.LATE >= fc.NSTEPS).all()
    # windows open at the start in some columns and not in others, among them columns that check later and columns that never do
    open0 = G["nleft0"] > 0.0
    assert (open0 & (once == 1)).any() and (open0 & never).any() and (~open0 & (sched >= 0)).any() and not (open0 & (sched < 0)).any()
    assert (G["rate0"][open0] > 0.0).all() and G["nleft0"].max() < ir.steps_per_day(fc.DT)


def test_the_storages_lie_on_both_sides_of_the_supply_threshold():
    """irrigation.supply_limit on the initial VOLR with every irrigated column checking at 2e-4 mm/s, a rate of the size the generated
    tier measures: cells that are cut back, cells that are granted in full, and the cases of the supply test's census that the map and
    the storages hold."""
    G = fc.geometry()
    ptr, col, w = G["map"]
    nspd = ir.steps_per_day(fc.DT)
    rate = np.where(G["sched"] >= 0, 2.0e-4, 0.0)
    nleft = np.where(G["sched"] >= 0, float(nspd), 0.0)
    rate_out, rows = ir.supply_limit(ptr, col, w, G["area"], G["volr"], rate, nleft, int(fc.DT), fc.THR, np.zeros(fc.NCELL))
    vd, ratio = rows[ir.DEMAND], rows[ir.RATIO]
    assert ((vd > 0.0) & (ratio < 1.0)).sum() >= 5 and ((vd > 0.0) & (ratio == 1.0)).sum() >= 5
    assert (ratio[G["low"]][vd[G["low"]] > 0.0] < 1.0).all()
    assert (rate_out < rate).any() and (rows[ir.UNMET_SUM] > 0.0).any()
    seen = sc.census(ptr, col, fc.NCOL, G["volr"], nleft, rate, nspd, rows)
    for k in ("empty_cell", "one_term_cell", "column_in_no_cell", "vd_below_avail", "vd_above_avail", "volr_negative"):
        assert seen[k] > 0, k


def test_the_storages_hold_the_paths_of_the_exchange_and_a_cell_crosses_its_bank():
    G = fc.geometry()
    tab = G["tab"]
    paths = ic.path_census(G["volr"], G["wf"], tab)
    names = {ic.PATHS[i] for i in paths}
    segments = {n for n in names if n.startswith("segment")}
    assert {"untouched", "returns", "above the profile"} <= names and len(segments) >= 3, names
    assert (G["wf"] > 0.0).any() and (G["wf"] == 0.0).any()
    # one call on network A without runoff: the hub, inside its banks with a dry floodplain, is over them afterwards
    hub = G["hub"]
    assert paths[hub] == 0 and G["volr"][hub] < tab["VC"][hub] and G["wf"][hub] == 0.0
    zero = np.zeros(fc.NCELL)
    out = rt.kinematic_call(G["wh"], G["wt"], G["volr"], zero, zero, G["area"], G["params"], rt.upstream_map(G["down_a"]), fc.DT, fc.NSUB_A,
                            flood=(tab, G["wf"]))
    volr1, wf1, frac1 = out[2], out[4], out[6]
    assert wf1[hub] > 0.0 and frac1[hub] > 0.0 and ic.path_census(volr1, wf1, tab)[hub] >= 2
    # ... and floodplains stay dry elsewhere
    assert (wf1 == 0.0).sum() >= 10 and (frac1 == 0.0).sum() >= 10
