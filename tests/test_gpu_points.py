"""The point series on the device (include/elmk.h "point series", P0 - P9): every kind of entry against the numpy restatement bit for bit
at the list sizes and map shapes the record kernel can go wrong at, the ring's order, elmk_run's records against the stand-alone calls
with a stepwise record after each step, the refusals and interlocks, the unchanged restart image, and the example."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import points as pt
from elmkernels_amd import regrid as RG
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import cell_history_cases as cc
from tests import full_step_cases as fc
from tests import heat_cases as hc
from tests import points_cases as pc
from tests import reservoir_cases as rc
from tests.run_cases import schedule, stepwise
from tests.support import build_demo, captured, run_demo, same

pytestmark = pytest.mark.gpu

LIBS = {"f64": None, "f32": L.F32_LIB_PATH}
BUILDS = ["f64", "f32"]
DT = 1800.0


# ---- a. gather entries over the columns ------------------------------------------------------------------------------------------------
def _column_context(build):
    """5003 columns of the irrigation's generated tier with the soil hydrology and the water balance on, one water balance call behind
    them (QRUNOFF holds values), and the special values in the columns the lists sample."""
    from tests.hydrology_cases import _new, clear_snow, prepare
    from tests.irrigation_cases import generated

    cols, scal, soil, _ = generated(pc.NCOL, 41)
    clear_snow(cols)
    rows = prepare(cols, 42)
    D = _new(cols, scal, soil, rows, LIBS[build])
    D.water_balance_enable(1.0e-9)
    D.upload("qflx_snwcp_liq", np.random.default_rng(43).uniform(0.0, 4.0e-5, pc.NCOL))
    D.water_balance(DT)
    at = np.unique(np.concatenate([pc.column_list(n) for n in pc.SIZES] + [np.array(pc.BASE_COLUMNS)]))
    t = D["t_soisno"]
    t[:, 0] = pc.plant_specials(t[:, 0], at)
    t[:, -1] = pc.plant_specials(t[:, -1], at[::-1][:at.size // 2])
    D["t_soisno"] = t
    D["err_flags"] = np.random.default_rng(44).integers(0, 2 ** 32, pc.NCOL, dtype=np.uint64).astype(np.uint32)
    D["veg_active"] = (np.arange(pc.NCOL) % 3 == 0).astype(np.uint8)
    return D


@pytest.fixture(scope="module")
def column_contexts():
    held = {}

    def get(build):
        if build not in held:
            held[build] = _column_context(build)
        return held[build]

    yield get
    for D in held.values():
        D.close()


COLUMN_ENTRIES = ("t_soisno/0", "t_soisno/last", "snl", "err_flags", "veg_active", "ZWT", "QRUNOFF")


def _add_column_entries(D):
    nlev = D.fields["t_soisno"][1]
    return [D.points_add_field("t_soisno", 0), D.points_add_field("t_soisno", nlev - 1), D.points_add_field("snl"),
            D.points_add_field("err_flags"), D.points_add_field("veg_active"), D.points_add_row("hydrology", hy.ZWT),
            D.points_add_row("water_balance", hy.WB_QRUNOFF)]


def _column_rows(D):
    t = D["t_soisno"]
    return {"t_soisno/0": np.ascontiguousarray(t[:, 0]), "t_soisno/last": np.ascontiguousarray(t[:, -1]), "snl": D["snl"],
            "err_flags": D["err_flags"], "veg_active": D["veg_active"], "ZWT": D.soil_hydrology_rows()[hy.ZWT],
            "QRUNOFF": D.water_balance_rows()[hy.WB_QRUNOFF]}


def _assert_entries(D, ids, names, want, rec, what):
    for e, name, w in zip(ids, names, want):
        got = D.points_read(e, rec, 1)
        assert got.shape == (1, w.size), (what, name)
        assert pc.same_bits(got[0], w), (what, name, np.nonzero(pc.words(got[0]) != pc.words(w))[0][:5])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", (len(pc.BASE_COLUMNS),) + pc.SIZES)
def test_gather_equals_the_restatement(column_contexts, n, build):
    """Seven entries - the first and the last level of t_soisno, snl, err_flags, a U8 field, ZWT and QRUNOFF - at lists of 6 (unsorted,
    with a duplicate), 1, 64, 65 and 257 points, NaN, -0.0 and the infinities among the samples: bit for bit."""
    D = column_contexts(build)
    D.points_clear()
    before = D.device_bytes
    lst = pc.column_list(n)
    D.points_set("columns", lst)
    ids = _add_column_entries(D)
    assert ids == list(range(len(COLUMN_ENTRIES)))
    D.points_reserve(3)
    assert D.device_bytes > before
    D.points_record(17.25)
    assert D.points_count() == (1, 1)
    rows = _column_rows(D)
    want = pt.record(rows, (lst, []), [(k, pt.COLUMNS, pt.GATHER) for k in COLUMN_ENTRIES])
    _assert_entries(D, ids, COLUMN_ENTRIES, want, 0, f"n = {n}")
    assert D.points_stamps().tolist() == [17.25]
    sampled = want[0]
    assert np.isnan(sampled).any() or n == 1
    if n >= 6:
        assert (np.isinf(sampled).any() and (pc.words(sampled) == pc.words(np.array([-0.0]))[0]).any()), "the specials are among the samples"
        assert want[3].max() > 2.0 ** 31 and want[5].any() and want[6].any()
    D.points_clear()
    assert D.device_bytes == before  # P8: everything is returned


# ---- b. cell rows --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def river_1001():
    return cc.river_case(330, pc.NCELL_ROWS, 60, cells_with_columns=100)


def _river_context(G, build=None, part=None):
    D = cc.context(G, LIBS.get(build), flood=False, supply=False)
    if part == "reservoir":
        dam = rc.dam_values(pc.NCELL_ROWS, 61)
        D.routing_reservoir_enable(*dam[:4])
        D.routing_reservoir_init(cc.finite(dam[4]), dam[5])
    if part == "heat":
        shade, tt, tr = hc.heat_values(pc.NCELL_ROWS, 62)
        D.routing_heat_enable(hc.SUBLEV, shade)
        D.routing_heat_init(*(np.where((x > 200.0) & (x < 400.0), x, 280.0) for x in (tt, tr)))
    return D


@pytest.mark.parametrize("part,which", [(None, (rt.VOLR, rt.QOUT)), ("reservoir", (rt.RES,)), ("heat", (rt.TR,))],
                         ids=["kinematic-VOLR-QOUT", "reservoir-RES", "heat-TR"])
def test_cell_rows_equal_routing_read(river_1001, part, which):
    """1001 cells (the cell stride is 1024), the cells 0, 1000, 63 and 64 among 65 and then one cell alone: a record before the first
    routing call holds the initial rows - their NaN, infinities and -0.0 included - and one after two steps the routing's result."""
    G = river_1001
    D = _river_context(G, None, part)
    cells = pc.cell_list(65)
    D.points_set("cells", cells)
    ids = [D.points_add_cell_row("routing", w) for w in which]
    D.points_reserve(4)
    D.points_record(1.0)
    first = [D.routing_read(w) for w in which]
    for k in range(2):
        cc.step(D, G, k, sample=False)
    D.points_record(2.0)
    second = [D.routing_read(w) for w in which]
    for e, a, b in zip(ids, first, second):
        got = D.points_read(e)
        assert got.shape == (2, 65) and pc.same_bits(got[0], a[cells]) and pc.same_bits(got[1], b[cells])
    assert not all(pc.same_bits(a, b) for a, b in zip(first, second)), "the routing moved the rows"
    # one cell, one entry
    D.points_clear()
    D.points_set("cells", [pc.NCELL_ROWS - 1])
    e = D.points_add_cell_row("routing", which[0])
    D.points_reserve(1)
    D.points_record(3.0)
    assert pc.same_bits(D.points_read(e)[0], second[0][[pc.NCELL_ROWS - 1]]) and D.points_stamps().tolist() == [3.0]
    D.close()


# ---- c. gridded entries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_gridded_equals_apply_aggregate(column_contexts, build):
    """5003 columns over 70 cells: a cell of 2100 terms (33 passes of 64), cells of exactly 64 and 65 terms, empty cells (fill), every
    cell sampled in a shuffled order with a duplicate; a field level and a feature row; beside a gather entry in the same launch."""
    D = column_contexts(build)
    D.points_clear()
    ptr, col, w = pc.grid_map()
    D["t_grnd"] = pc.wide_row(pc.NCOL, 45)
    D.set_output_grid(ptr, col, w, fill=pc.FILL)
    cells = np.concatenate([np.random.default_rng(46).permutation(pc.NCELL_GRID), [pc.BIG]])
    D.points_set("cells", cells)
    D.points_set("columns", pc.column_list(65))
    ids = [D.points_add_gridded_field("t_grnd"), D.points_add_field("snl"), D.points_add_gridded_row("hydrology", hy.ZWT),
           D.points_add_gridded_field("snl")]
    D.points_reserve(2)
    D.points_record(0.5)
    rows = {"t_grnd": D["t_grnd"], "snl": D["snl"], "ZWT": D.soil_hydrology_rows()[hy.ZWT]}
    entries = [("t_grnd", pt.CELLS, pt.GRIDDED), ("snl", pt.COLUMNS, pt.GATHER), ("ZWT", pt.CELLS, pt.GRIDDED), ("snl", pt.CELLS, pt.GRIDDED)]
    want = pt.record(rows, (pc.column_list(65), cells), entries, (ptr, col, w, pc.FILL))
    _assert_entries(D, ids, [e[0] for e in entries], want, 0, "gridded")
    assert pc.same_bits(want[0], RG.apply_aggregate(ptr, col, w, rows["t_grnd"], pc.FILL)[cells])
    assert pc.same_bits(D.points_read(ids[0])[0], D.download_gridded("t_grnd")[cells])  # P2: elmk_download_gridded's value
    empty = np.isin(cells, pc.EMPTY)
    assert empty.sum() == len(pc.EMPTY) and (want[0][empty] == pc.FILL).all() and (want[0][~empty] != pc.FILL).all()
    # the interlock of P7 under gridded entries and a cells list, then the way out
    for call in (D.clear_output_grid, lambda: D.set_output_grid(ptr, col, w, fill=0.0)):
        with pytest.raises(L.ElmkError, match="elmk_points_clear first"):
            call()
    assert pc.same_bits(D.points_read(ids[0])[0], want[0])
    D.points_clear()
    D.clear_output_grid()


# ---- d. the ring ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", BUILDS)
def test_ring_keeps_the_last_records_in_order(column_contexts, build):
    D = column_contexts(build)
    D.points_clear()
    lst = pc.column_list(65)
    D.points_set("columns", lst)
    e, s = D.points_add_field("t_grnd"), D.points_add_field("snl")
    D.points_reserve(4)
    assert D.points_count() == (0, 0) and D.points_read(e).shape == (0, 65)
    states = []
    for k in range(6):
        D["t_grnd"] = 250.0 + k + 0.001 * np.arange(pc.NCOL)
        states.append(D["t_grnd"][lst])
        D.points_record(100.0 + k)
        total, held = D.points_count()
        records, _ = pt.ring(total, 4)
        assert (total, held) == (k + 1, min(k + 1, 4)) and records.size == held
    got = D.points_read(e)
    assert got.shape == (4, 65) and all(pc.same_bits(got[j], states[2 + j]) for j in range(4))
    assert D.points_stamps().tolist() == [102.0, 103.0, 104.0, 105.0]
    assert pc.same_bits(D.points_read(e, 1, 2), np.stack(states[3:5])) and D.points_stamps(3, 1).tolist() == [105.0]
    assert pc.same_bits(D.points_read(s, 3, 1)[0], D["snl"][lst].astype(np.float64))
    with pytest.raises(L.ElmkError, match="bad record range"):
        D.points_read(e, 2, 3)
    D.points_reset()
    assert D.points_count() == (0, 0)
    D.points_record(7.0)
    assert D.points_count() == (1, 1) and D.points_stamps().tolist() == [7.0] and pc.same_bits(D.points_read(e)[0], states[5])
    D.points_clear()


# ---- e. elmk_run against the stand-alone calls ---------------------------------------------------------------------------------------
RUN_NAMES = ("t_grnd", "t_soisno/5", "ZWT", "QRUNOFF", "QOUT", "VOLR", "WF", "g:t_grnd", "g:QRUNOFF")


def _arm(D, G):
    """Three columns and three cells - the hub of network A, which floods during the run, its first source and the last cell - with an
    entry of every kind; sixteen records."""
    D.points_set("columns", [0, fc.NCOL - 1, 64])
    D.points_set("cells", [G["hub"], int(G["srcs"][0]), fc.NCELL - 1])
    ids = [D.points_add_field("t_grnd"), D.points_add_field("t_soisno", 5), D.points_add_row("hydrology", hy.ZWT),
           D.points_add_row("water_balance", hy.WB_QRUNOFF), D.points_add_cell_row("routing", rt.QOUT),
           D.points_add_cell_row("routing", rt.VOLR), D.points_add_cell_row("routing", rt.WF), D.points_add_gridded_field("t_grnd"),
           D.points_add_gridded_row("water_balance", hy.WB_QRUNOFF)]
    D.points_reserve(16)
    return ids


def _series(D, ids):
    return [D.points_read(e) for e in ids] + [D.points_stamps()]


# the steps of the twelve that record: 0 - 5 (two runs of three), 6 - 7, not 8 - 9 (set_run(0)), 10 - 11 (on again)
RECORDED = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11)
EXTRA_STAMP = 99.0  # the stepwise record between the second and the third run


@pytest.fixture(scope="module")
def stepwise_series():
    """Per build, once: the full context stepped through the stand-alone calls with elmk_points_record(decday) after each recorded step
    and the extra record after step 5: the series, and the snapshot after step 9."""
    out = {}

    def get(build):
        if build not in out:
            G = fc.case()
            steps = schedule(fc.NSTEPS)
            A = fc.full_context(False, LIBS[build])
            ids = _arm(A, G)
            shot = None
            for s in range(fc.NSTEPS):
                stepwise(A, G["rec"], steps[s:s + 1], fc.ALL_FLAGS, fc.DT, rec_times=fc.REC_TIMES)
                if s in RECORDED:
                    A.points_record(float(steps[s]["decday"]))
                if s == 5:
                    A.points_record(EXTRA_STAMP)
                if s == 9:
                    shot = {k: A[k] for k in ("t_grnd", "t_soisno", "h2osoi_liq")}
                    shot["VOLR"] = A.routing_read(rt.VOLR)
            out[build] = (_series(A, ids), shot)
            A.close()
        return out[build]

    return get


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_records_what_stepwise_records(stepwise_series, graph, build):
    """P5, P6, P9.  Two runs of three steps enqueued back to back give the series of six; a stepwise record between two runs keeps the
    numbering; with set_run(0) a run records nothing and leaves the state, tapes and diagnostics of a context that never had the part;
    switched on again the series goes on.  With the graph on the later runs replay the step the first captured: the slot is not in it."""
    want, shot = stepwise_series(build)
    G = fc.case()
    steps = schedule(fc.NSTEPS)
    B = fc.full_context(graph, LIBS[build])
    C = fc.full_context(graph, LIBS[build])  # never has the part
    ids = _arm(B, G)
    B.points_set_run(True)
    fc.run(B, steps[0:3])
    fc.run(B, steps[3:6])
    assert B.points_count() == (6, 6)  # (known on the host: nothing has been waited for)
    B.points_record(EXTRA_STAMP)
    fc.run(B, steps[6:8])
    assert B.points_count() == (9, 9)
    B.points_set_run(False)
    fc.run(B, steps[8:10])
    assert B.points_count() == (9, 9)
    for lo, hi in ((0, 3), (3, 6), (6, 8), (8, 10)):
        fc.run(C, steps[lo:hi])
    fc.assert_same_snapshot(fc.full_snapshot(B), fc.full_snapshot(C), "a run with the part switched off")
    assert same(B["t_grnd"], shot["t_grnd"]) and same(B["t_soisno"], shot["t_soisno"]) and same(B.routing_read(rt.VOLR), shot["VOLR"])
    B.points_set_run(True)
    fc.run(B, steps[10:12])
    assert B.points_count() == (11, 11)
    got = _series(B, ids)
    for name, g, w in zip(RUN_NAMES + ("stamps",), got, want):
        assert g.shape == w.shape and pc.same_bits(g, w), (name, np.argwhere(pc.words(g) != pc.words(w))[:4])
    stamps = [float(steps[s]["decday"]) for s in RECORDED]
    assert got[-1].tolist() == stamps[:6] + [EXTRA_STAMP] + stamps[6:]
    # the series is one of a river that moved: the hub's discharge and storage differ from step to step, and the hub flooded
    qout, volr, wf = got[4][:, 0], got[5][:, 0], got[6][:, 0]
    assert np.unique(qout).size > 3 and np.unique(volr).size > 3 and (wf > 0.0).any()
    assert np.unique(got[0][:, 0]).size > 3
    B.close()
    C.close()


# ---- f. refusals and interlocks --------------------------------------------------------------------------------------------------------
def _refused(D, text, call, before):
    with pytest.raises(L.ElmkError, match=text):
        call()
    assert (D.points_count(), D.device_bytes) == before, text


@pytest.mark.parametrize("build", ["f64"])
def test_refusals_change_nothing(column_contexts, build):
    D = column_contexts(build)
    D.points_clear()
    lst = pc.column_list(65)
    state = lambda: (D.points_count(), D.device_bytes)  # noqa: E731
    # P4: nothing to record yet
    _refused(D, "elmk_points_record: no reservation", lambda: D.points_record(1.0), state())
    _refused(D, "elmk_points_set_run: no reservation", lambda: D.points_set_run(True), state())
    D.points_reserve(4)
    _refused(D, "elmk_points_record: no entries", lambda: D.points_record(1.0), state())
    e = D.points_add_field("t_grnd")
    _refused(D, "elmk_points_record: an entry's columns list is empty", lambda: D.points_record(1.0), state())
    D.points_set("columns", lst)
    # P0: the sources the history entry points refuse
    nlev = D.fields["t_soisno"][1]
    for text, call in (("elmk_points_add_field: unknown field", lambda: D.points_add_field(-1)),
                       ("elmk_points_add_field: unknown field", lambda: D.points_add_field(100000)),
                       ("elmk_points_add_field: level out of range", lambda: D.points_add_field("t_soisno", nlev)),
                       ("elmk_points_add_field: level out of range", lambda: D.points_add_field("t_grnd", -1)),
                       ("elmk_points_add_row: the family's feature is not enabled", lambda: D.points_add_row("frost", 0)),
                       ("elmk_points_add_row: unknown row$", lambda: D.points_add_row("hydrology", hy.NROWS)),
                       ("elmk_points_add_row: unknown row family", lambda: D.points_add_row(-1, 0)),
                       ("elmk_points_add_row: unknown row family", lambda: D.points_add_row(5, 0)),
                       ("elmk_points_add_cell_row: unknown cell-row family", lambda: D.points_add_cell_row(2, 0)),
                       ("elmk_points_add_cell_row: .*elmk_routing_enable", lambda: D.points_add_cell_row("routing", rt.VOLR)),
                       ("elmk_points_add_gridded_field: no output grid", lambda: D.points_add_gridded_field("t_grnd")),
                       ("elmk_points_add_gridded_row: no output grid", lambda: D.points_add_gridded_row("hydrology", hy.ZWT)),
                       ("elmk_points_set: no output grid", lambda: D.points_set("cells", [0])),
                       ("elmk_points_set: unknown kind", lambda: D.points_set(2, [0])),
                       # P7: the first offending position and value
                       (r"elmk_points_set: idx\[2\] = 5003 outside 0 \.\. ncols - 1", lambda: D.points_set("columns", [0, 5002, pc.NCOL, -1])),
                       (r"elmk_points_set: idx\[1\] = -1 outside", lambda: D.points_set("columns", [0, -1, pc.NCOL])),
                       ("elmk_points_set: n outside", lambda: D.points_set("columns", np.zeros(pt.MAX_POINTS + 1, np.int64))),
                       ("elmk_points_reserve: need 1 <= max_records", lambda: D.points_reserve(0))):
        _refused(D, text, call, state())
    with captured(D):
        for text, call in (("elmk_points_record: the stream is being captured", lambda: D.points_record(1.0)),
                           ("elmk_points_add_field: the stream is being captured", lambda: D.points_add_field("snl")),
                           ("elmk_points_set: the stream is being captured", lambda: D.points_set("columns", [1]))):
            with pytest.raises(L.ElmkError, match=text):
                call()
    assert D.points_count() == (0, 0)
    # the lists and the entry are what they were: a record gives their values
    D.points_record(1.0)
    want = D["t_grnd"][lst]
    assert pc.same_bits(D.points_read(e)[0], want)
    # entries and lists stay while total > 0
    for text, call in (("elmk_points_add_field: the series holds records", lambda: D.points_add_field("snl")),
                       ("elmk_points_set: the series holds records", lambda: D.points_set("columns", [1])),
                       ("elmk_points_reserve: the series holds records", lambda: D.points_reserve(8))):
        _refused(D, text, call, state())
    assert pc.same_bits(D.points_read(e)[0], want) and D.points_count() == (1, 1)
    D.points_reset()
    # the 65th entry
    for k in range(pt.MAX_ENTRIES - 1):
        assert D.points_add_field("t_soisno", k % nlev) == k + 1
    _refused(D, "elmk_points_add_field: the entry table is full", lambda: D.points_add_field("snl"), state())
    D.points_set("columns", np.arange(pt.MAX_POINTS))  # 64 entries x 4096 points: the largest record
    D.points_record(2.0)
    t = D["t_soisno"]
    assert pc.same_bits(D.points_read(pt.MAX_ENTRIES - 1)[0], t[:pt.MAX_POINTS, (pt.MAX_ENTRIES - 2) % nlev])
    assert pc.same_bits(D.points_read(0)[0], D["t_grnd"][:pt.MAX_POINTS])
    D.points_clear()


def test_guarded_clears(column_contexts, river_1001):
    """P7: while an entry reads rows, the clear that would free them is refused and changes nothing; after elmk_points_clear it is not."""
    D = column_contexts("f64")
    D.points_clear()
    D.points_set("columns", [3])
    D.points_add_row("water_balance", hy.WB_QRUNOFF)
    wb = D.water_balance_rows()
    with pytest.raises(L.ElmkError, match="elmk_water_balance_clear: point-series entries over its rows exist .elmk_points_clear first"):
        D.water_balance_clear()
    with pytest.raises(L.ElmkError, match="elmk_soil_hydrology_clear: point-series entries .*elmk_points_clear first"):
        D.soil_hydrology_clear()
    assert same(D.water_balance_rows(), wb)
    D.points_clear()
    D.points_add_row("hydrology", hy.ZWT)
    D.water_balance_clear()  # (no entry reads its rows now)
    with pytest.raises(L.ElmkError, match="elmk_soil_hydrology_clear: point-series entries .*elmk_points_clear first"):
        D.soil_hydrology_clear()
    D.points_clear()
    D.water_balance_enable(1.0e-9)
    D.water_balance(DT)  # (the contexts are shared: QRUNOFF holds values again)
    # the river's rows
    R = _river_context(river_1001)
    R.points_set("cells", [0, pc.NCELL_ROWS - 1])
    R.points_add_cell_row("routing", rt.WH)
    R.points_reserve(2)
    with pytest.raises(L.ElmkError, match="elmk_points_set: idx.0. = 1001 outside 0 .. ncells - 1"):
        R.points_set("cells", [pc.NCELL_ROWS])
    R.points_record(1.0)
    held = R.points_read(0)
    for text, call in (("elmk_routing_clear", R.routing_clear), ("elmk_routing_kinematic_clear", R.routing_kinematic_clear),
                       ("elmk_clear_output_grid", R.clear_output_grid),
                       ("elmk_set_output_grid", lambda: R.set_output_grid(*river_1001["map"], fill=0.0))):
        with pytest.raises(L.ElmkError, match=text + ": .*elmk_points_clear first"):
            call()
    assert pc.same_bits(R.points_read(0), held) and pc.same_bits(held[0], R.routing_read(rt.WH)[[0, pc.NCELL_ROWS - 1]])
    R.points_clear()
    R.routing_kinematic_clear()
    R.routing_clear()
    R.close()


# ---- g. the image, the example -------------------------------------------------------------------------------------------------------
def test_image_is_the_image_without_the_part():
    """P8: a context that records - stepwise and in a run - saves byte for byte the image of one that never had the part."""
    G = fc.case()
    steps = schedule(fc.NSTEPS)
    imgs = []
    for part in (True, False):
        D = fc.full_context(True)
        if part:
            _arm(D, G)
            D.points_set_run(True)
        fc.run(D, steps[:2])
        if part:
            D.points_record(5.0)
            assert D.points_count() == (3, 3)
        imgs.append(D.restart_save())
        D.close()
    assert imgs[0].size == imgs[1].size and same(imgs[0], imgs[1])


def test_point_series_demo_runs(tmp_path):
    r = run_demo(build_demo("point_series_demo", tmp_path))
    assert "hydrograph" in r.stdout and "OK" in r.stdout
