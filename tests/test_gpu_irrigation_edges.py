"""The irrigation on the device on its edge tier (tests/irrigation_cases.py: edge_tier; tests/irrigation_supply_cases.py: shape_map):
k_irrigation<false> and k_irrigation_supply against the host restatements (irrigation.step, irrigation.supply_limit) bit for bit in both
builds - every column and every cell of every row, a NaN by its bits (the rows are canonical on both sides, and a NaN of a state field
is the one that was uploaded) - at the sizes of a ragged last wave, at step lengths that give every nspd from 14400 down to 1, and on
every map shape the limit's tiles and workgroups can go wrong at; then k_irrigation<true> and k_active_layer<true> on the pad word they
share, and the run's clock at a step that does not divide the day, against the stepwise calls.  tests/test_irrigation_edges_host.py
shows on the CPU that the censuses asserted here can be met and that a one-character slip of the statement changes these results.

No wrapper runs between the upload of the tier and elmk_irrigation: the seven wrappers overwrite btran and the two precipitation terms."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import active_layer as al
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests import irrigation_cases as IC
from tests import irrigation_supply_cases as SC
from tests.hydrology_cases import _new, clear_snow, prepare
from tests.run_cases import NREC, SERIES, _inputs, same, schedule, upload_series
from tests.support import bits

pytestmark = pytest.mark.gpu

LIBS = pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
TOL = 1.0e-9
NAN, INF = float("nan"), float("inf")
SUP = (ir.DEMAND, ir.COMMITTED, ir.RATIO, ir.UNMET_SUM)


def _first(got, want, n):
    """The first column that differs, its edge class and the two values: what an assertion shows."""
    g, w = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    bad = np.nonzero(g.view(np.uint64) != w.view(np.uint64))[0]
    if not bad.size:
        return None
    i = int(bad[0])
    names = [c[0] for c in IC.edge_classes()]
    return i, (names[i // 2] if i % 2 == 0 and i // 2 < len(names) else "ordinary"), g[i].tolist(), w[i].tolist(), int(bad.size)


def _chain_on_the_device(n, dt, lib_path):
    """The edge tier uploaded once, the rows seeded through elmk_irrigation_init, then the chain of clock_tods(dt) with nothing in
    between: after every call the three rows and the two state fields against irrigation.step on what the device held before it;
    what the stage reads is only read, and in the first and the last call every other field is untouched as well.  Returns the census."""
    cols, scal, soil, sched = IC.edge_tier(n, 900)
    lat, lon = synth.global_grid(n, seed=9)
    D = H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)
    D.irrigation_enable(sched)
    D.irrigation_init(*IC.edge_seed(n, dt))
    smpso = IC.smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    seen = {}
    rows = D.irrigation_rows()
    assert bits(rows[:2]) == bits(np.stack(IC.edge_seed(n, dt)))
    tods = IC.clock_tods(dt)
    for s, tod in enumerate(tods):
        fields = {k: D[k] for k in ir.READS}
        want, want_rows = IC.edge_step(seen, fields, rows, sched, float(dt), tod, smpso, stored=stored)
        everything = s in (0, len(tods) - 1)
        others = {k: D[k] for k in D.fields if k not in ir.WRITES} if everything else {k: v for k, v in fields.items() if k not in ir.WRITES}
        D.irrigation(float(dt), tod)
        rows = D.irrigation_rows()
        for w in range(ir.NROWS):
            assert bits(rows[w]) == bits(want_rows[w]), (dt, s, tod, "row", w, _first(rows[w], want_rows[w], n))
        for k in ir.WRITES:
            assert same(D[k], want[k]), (dt, s, tod, k, _first(D[k], want[k], n))
        for k, v in others.items():
            assert same(D[k], v), (dt, s, tod, k, "touched")
    D.close()
    return seen


# ---- 1, 2. the stage on the edge tier -------------------------------------------------------------------------------------------------
@LIBS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1001])
def test_the_edge_tier_equals_the_restatement(n, lib_path):
    """One column (an edge column that checks), a wave less one, a wave, a wave and one, 257 columns (every edge class once, two
    workgroups, the last with one column) and 1001, at dt = 1800.  From 257 columns on the census is complete."""
    seen = _chain_on_the_device(n, 1800, lib_path)
    print(f"n={n} census: {seen}")
    assert seen.get("check", 0) > 0
    if n >= 257:
        assert not IC.census_missing(seen, 1800), IC.census_missing(seen, 1800)


@LIBS
@pytest.mark.parametrize("dt", IC.DTS)
def test_the_edge_tier_at_other_step_lengths(dt, lib_path):
    """257 columns at dt = 1 (nspd 14400), 1800, 3600, 7000 (no divisor of the window: nspd 3), 14400, 14401 (a step longer than
    the window) and 86400 (every clock is in: off_clock and since_first_out cannot occur and are exempt).  The seeded rows open
    and close the windows the short chain cannot: at dt = 1 window_ran_out comes from the seeded NLEFT 1 and 2."""
    seen = _chain_on_the_device(257, dt, lib_path)
    print(f"dt={dt} census: {seen}")
    assert not IC.census_missing(seen, dt), IC.census_missing(seen, dt)


# ---- 3, 4. the limit --------------------------------------------------------------------------------------------------------------------
LEADS = ("sucsat[2]=nan", "h2osoi_liq[7]=-inf", "dz[7]=1e+300", "eff_porosity[2]=inf", "t_soisno[5]=0.0")
LIMIT_TODS = (21600, 0, 43200, 21600)  # the sched 0 columns check in the first and the last call, the others in between


def _limit_context(ptr, col, w, ncols, lib_path, thr, seed=900):
    """The edge tier over `ncols` columns with the soil hydrology and the water balance (the routing needs them; their rows are those
    of a copy, so that the tier stays what it is), the map as the output grid, the irrigation, the routing with every cell an outlet
    and the withdrawal on, and the limit."""
    cols, scal, soil, sched = IC.edge_tier(ncols, seed)
    rows0 = prepare({k: np.array(v) for k, v in cols.items()}, 614)
    ncells = ptr.size - 1
    area, _ = SC.cell_values(ncells, 52)
    D = _new(cols, scal, soil, rows0, lib_path)
    D.water_balance_enable(TOL)
    D.set_output_grid(ptr, col, w, fill=NAN)
    D.irrigation_enable(sched)
    D.routing_enable(np.full(ncells, -1, np.int32), np.full(ncells, 5.0e4), area, rt.EFFVEL, 1)
    D.routing_set_withdrawal(True)
    D.irrigation_supply_enable(thr)
    return D, cols, sched, area


def _limit_call(D, m, ncols, sched, smpso, stored, area, volr, rows, unmet, dt, thr, tod, everything, what):
    """VOLR set, one elmk_irrigation with the limit behind it, and everything it leaves against irrigation.step followed by
    irrigation.supply_limit on what the device held.  Returns the rows, the cell rows and what the two restatements gave."""
    ptr, col, w = m
    D.routing_init(volr)
    fields = {k: D[k] for k in ir.READS}
    others = {k: D[k] for k in D.fields if k not in ir.WRITES} if everything else {k: v for k, v in fields.items() if k not in ir.WRITES}
    want_f, want = ir.step(fields, rows, sched, float(dt), tod, smpso, stored=stored)
    want_rate, want_sup = ir.supply_limit(ptr, col, w, area, volr, want[ir.RATE], want[ir.NLEFT], int(dt), thr, unmet, qflx_irrig=want[ir.QFLX_IRRIG])
    D.irrigation(float(dt), tod)
    got, sup = D.irrigation_rows(), np.stack([D.irrigation_supply_read(k) for k in SUP])
    assert bits(got[ir.RATE]) == bits(want_rate), (what, "RATE", _first(got[ir.RATE], want_rate, ncols))
    assert bits(got[ir.NLEFT]) == bits(want[ir.NLEFT]) and bits(got[ir.QFLX_IRRIG]) == bits(want[ir.QFLX_IRRIG]), what
    for k in SUP:
        bad = np.nonzero(sup[k].view(np.uint64) != want_sup[k].view(np.uint64))[0]
        assert not bad.size, (what, "cell row", k, bad[:5].tolist(), sup[k][bad[:5]].tolist(), want_sup[k][bad[:5]].tolist())
    for k in ir.WRITES:
        assert same(D[k], want_f[k]), (what, k)
    for k, v in others.items():
        assert same(D[k], v), (what, k, "touched")
    assert bits(D.routing_read(rt.VOLR)) == bits(volr), what  # (the limit only reads it)
    return got, sup, want, want_rate, want_sup


@pytest.mark.parametrize("thr", [0.0, 0.1])
@pytest.mark.parametrize("dt", [1, 1800, 7000, 86400])
@LIBS
def test_the_limit_behind_the_edge_tier(lib_path, dt, thr):
    """129 cells in three workgroups over just enough columns of the edge tier: cell 63, the last of its workgroup, holds 2100
    columns, cells 64 .. 127 are a workgroup without a term, five edge columns whose checks give a NaN, a +inf, a huge and a zero
    rate lead cells of their own.  Four calls; RATE, NLEFT and UNMET_SUM chain; the storages are drawn anew before every call with
    the edge storages in cells 8 .. 13, and in the first call the cell of the +inf rate holds an infinite storage, so that the rate
    survives to be committed in the second and is cut to NaN (inf x 0) when the column checks again in the last.  The NaN and inf
    rates the limit sums are produced by k_irrigation in the same call.  Both censuses are complete over the four calls."""
    lead = [IC.edge_index(name, 10 ** 6) for name in LEADS]
    ptr, col, w, ncols = SC.shape_map(129, 77, "big_last", lead=lead)
    m = (ptr, col, w)
    D, cols, sched, area = _limit_context(ptr, col, w, ncols, lib_path, thr)
    nspd = ir.steps_per_day(dt)
    rate0, nleft0 = IC.edge_seed(ncols, dt)
    c = np.arange(ncols)
    nleft0 = np.where((c % 2 == 1) & (c // 2 % 4 == 1), float(nspd + 2), nleft0)  # open windows on ordinary columns at every nspd
    D.irrigation_init(rate0, nleft0)
    smpso = IC.smpso_of(cols["vtype"])
    stored = np.float32 if lib_path else None
    rows, unmet = D.irrigation_rows(), np.zeros(129)
    seen, edge = dict.fromkeys(SC.CASES, 0), dict.fromkeys(SC.SUPPLY_EDGE_CASES, 0)
    inf_cell = int(SC.cell_of_column(ptr, col, ncols)[lead[1]])
    for s, tod in enumerate(LIMIT_TODS):
        _, volr = SC.cell_values(129, 60 + s, lo=2.0 + 0.5 * s, hi=7.0)
        if s == 0:
            volr[inf_cell] = INF
        rows, sup, want, want_rate, want_sup = _limit_call(D, m, ncols, sched, smpso, stored, area, volr, rows, unmet, dt, thr, tod, s == 0, (dt, thr, s))
        for k, v in SC.census(ptr, col, ncols, volr, want[ir.NLEFT], want[ir.RATE], nspd, want_sup).items():
            seen[k] += v
        for k, v in SC.supply_edge_census(ptr, col, ncols, want[ir.NLEFT], want[ir.RATE], want_rate, nspd, want_sup).items():
            edge[k] += v
        unmet = sup[ir.UNMET_SUM]
    print(f"dt={dt} thr={thr} census over four calls: {seen} edge census: {edge}")
    assert all(seen[k] > 0 for k in SC.CASES), [k for k in SC.CASES if not seen[k]]
    assert all(edge[k] > 0 for k in SC.SUPPLY_EDGE_CASES), [k for k in SC.SUPPLY_EDGE_CASES if not edge[k]]
    D.close()


@pytest.mark.parametrize("layout", ["tiles", "big_last"])
@pytest.mark.parametrize("ncells", [1, 63, 64, 65, 129])
def test_the_limit_on_every_map_shape(ncells, layout):
    """One cell, a workgroup less one, a workgroup, a workgroup and one cell, two and one; "tiles": the first workgroup's span is
    exactly one LDS tile (1024 terms) and the second's one term more; "big_last": the last cell of the first workgroup spans more
    than two tiles and the second workgroup has no term (P0 == P1).  Two calls each at dt = 1800, the fp64 build."""
    ptr, col, w, ncols = SC.shape_map(ncells, 78, layout)
    D, cols, sched, area = _limit_context(ptr, col, w, ncols, None, 0.1)
    D.irrigation_init(*IC.edge_seed(ncols, 1800))
    smpso = IC.smpso_of(cols["vtype"])
    rows, unmet = D.irrigation_rows(), np.zeros(ncells)
    limited = 0
    for s, tod in enumerate(LIMIT_TODS[:2]):
        _, volr = SC.cell_values(ncells, 60 + s, lo=2.0, hi=7.0)
        rows, sup, want, want_rate, _ = _limit_call(D, (ptr, col, w), ncols, sched, smpso, None, area, volr, rows, unmet, 1800, 0.1, tod, s == 0,
                                                   (ncells, layout, s))
        limited += int((want_rate.view(np.uint64) != want[ir.RATE].view(np.uint64)).sum())
        unmet = sup[ir.UNMET_SUM]
    assert limited > 0
    D.close()


def test_the_limit_on_a_map_without_a_term():
    """129 cells, none with a term: the limit's launch runs over three workgroups of empty spans.  DEMAND, COMMITTED and UNMET_SUM
    stay +0.0, RATIO is S4's 1.0 (Vd = 0 is not above avail), and RATE is the irrigation's own."""
    ptr, col, w, ncols = SC.shape_map(129, 78, "all_empty")
    D, cols, sched, area = _limit_context(ptr, col, w, ncols, None, 0.1)
    D.irrigation_init(*IC.edge_seed(ncols, 1800))
    smpso = IC.smpso_of(cols["vtype"])
    rows, unmet = D.irrigation_rows(), np.zeros(129)
    for s, tod in enumerate(LIMIT_TODS[:2]):
        _, volr = SC.cell_values(129, 60 + s)
        rows, sup, want, want_rate, _ = _limit_call(D, (ptr, col, w), ncols, sched, smpso, None, area, volr, rows, unmet, 1800, 0.1, tod, s == 0, s)
        assert bits(rows[ir.RATE]) == bits(want[ir.RATE]) and (want[ir.NLEFT] == 8.0).any()
        for k in (ir.DEMAND, ir.COMMITTED, ir.UNMET_SUM):
            assert bits(sup[k]) == bits(np.zeros(129)), k
        assert bits(sup[ir.RATIO]) == bits(np.ones(129))
        unmet = sup[ir.UNMET_SUM]
    D.close()


# ---- 5. the pad word of the run's step table ----------------------------------------------------------------------------------------------
NCOL = 193
NSTEPS = 8
ROLL_STEP = 4
ALT_FLAGS = st.RUN_ALT | st.RUN_IRRIGATION | st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE
ALT_ROWS = (al.ALT, al.ALTMAX, al.ALTMAX_LASTYEAR)


def rollover_schedule(day0, nsteps=NSTEPS):
    """Half-hour steps from 22:00 of day `day0` of the year (0-based): step 4 starts at 00:00 of the next day.  day0 = 364 crosses
    1 January (doy 364 -> 0, decday -> 1.0: the northern rollover), day0 = 180 crosses 1 July (doy 180 -> 181, decday -> 182.0: the
    southern one)."""
    S = schedule(nsteps)
    for s in range(nsteps):
        ddoy = ((day0 * 48 + 44 + s) % (365 * 48)) / 48.0
        S[s]["decday"], S[s]["doy"] = ddoy + 1.0, int(ddoy)
    roll = [al.rollover(int(p["doy"]), float(p["decday"])) for p in S]
    assert roll == [0] * ROLL_STEP + [al.ROLL_NORTH if day0 == 364 else al.ROLL_SOUTH] + [0] * (nsteps - ROLL_STEP - 1)
    tods = [ir.time_of_day(float(p["decday"]), int(p["doy"])) for p in S]
    assert tods == [(79200 + 1800 * s) % 86400 for s in range(nsteps)] and tods[ROLL_STEP] == 0
    return S


@pytest.fixture(scope="module")
def alt_base():
    b = list(_inputs(NCOL, 531))
    cols = b[0]
    clear_snow(cols)
    rows = prepare(cols, 532)
    c = np.arange(NCOL)
    # a thaw front in most columns (test_gpu_active_layer.py's), thawed at the top so that the irrigation measures a deficit
    rng = np.random.default_rng(5)
    t = al.TFRZ + 6.0 * rng.random((NCOL, 1)) - 0.6 * np.arange(20)[None, :] + 4.0
    t[::9] = 262.0
    t[4::9] = 281.0
    cols["t_soisno"] = t
    cols["altmax_indx"] = np.full(NCOL, 5, np.int32)
    cols["altmax_lastyear_indx"] = np.zeros(NCOL, np.int32)
    lat = np.array(b[3])
    lat[10], lat[11] = 0.0, -0.0
    b[3] = lat
    assert al.north(lat).sum() > 40 and (~al.north(lat)).sum() > 40 and not al.north(lat[10:12]).any()
    # column c passes 06:00 local in step 2 + c % 6 of rollover_schedule: before, in and after the rollover step; one in seven is not irrigated
    tod = (79200 + 1800 * (2 + c % 6)) % 86400
    sched = ((ir.IRRIG_START - tod + 100 * (c % 5)) % 86400).astype(np.int32)
    sched[c % 7 == 3] = -1
    return tuple(b), rows, sched


def _altmax0(n):
    return 0.01 * np.arange(n), 5.0 - 0.02 * np.arange(n)


def _alt_context(base, graph, sched=None, alt=True, irrig=True):
    b, rows, sched0 = base
    D = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    if irrig:
        D.irrigation_enable(sched0 if sched is None else sched)
    if alt:
        D.active_layer_enable()
        D.active_layer_init(*_altmax0(NCOL))
    return D


def _physics_inputs(D, rec, p, dt):
    D.solar_geometry(dt, float(p["decday"]), int(p["doy"]))
    f = int(p["forc_slot"])
    for k in st.SERIES_FORCING:
        D.upload(k, np.stack([rec[k][f], rec[k][f + 1]], axis=1))
    for k in st.SERIES_PHENOLOGY:
        D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
    st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
    st.get_forcing(D, p["forc_wt1"], p["forc_wt2"], False)
    st.kokkos_init_timestep(D)


def _alt_stepwise(D, rec, steps, dt=1800.0):
    """The stand-alone calls in elmk_run's documented order: the step's inputs, W0, the fused seven, elmk_irrigation at
    irrigation.time_of_day, the rest of the physics, the soil hydrology, conservation, the flag summary, W1 - W8, then
    elmk_active_layer_update with the step's rollover.  Returns ALTMAX_LASTYEAR and NLEFT after every step."""
    lastyear, nleft = [], []
    for p in steps:
        _physics_inputs(D, rec, p, dt)
        D.water_balance_begin()
        st.timestep7_fused(D, dt)
        D.irrigation(dt, ir.time_of_day(float(p["decday"]), int(p["doy"])))
        st.kokkos_soil_temperature(D, dt)
        st.kokkos_snow_hydrology(D, dt)
        st.kokkos_surface_fluxes(D, dt)
        D.soil_hydrology(dt)
        st.kokkos_evaluate_conservation(D, dt)
        D.error_summary()
        D.water_balance(dt)
        D.active_layer_update(al.rollover(int(p["doy"]), float(p["decday"])))
        lastyear.append(D.active_layer_read(al.ALTMAX_LASTYEAR))
        nleft.append(D.irrigation_read(ir.NLEFT))
    return np.array(lastyear), np.array(nleft)


def _alt_snapshot(D, alt=True, irrig=True):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out["hyd"], out["wb"] = D.soil_hydrology_rows(), D.water_balance_rows()
    if irrig:
        out["irr"] = D.irrigation_rows()
    if alt:
        out["alt"] = np.stack([D.active_layer_read(w) for w in ALT_ROWS])
    return out


def _assert_same(a, b, what=""):
    assert a.keys() == b.keys()
    for k, v in a.items():
        assert same(v, b[k]), (what, k)


@pytest.fixture(scope="module")
def alt_stepwise_result(alt_base):
    out = {}
    for day0 in (364, 180):
        A = _alt_context(alt_base, False)
        lastyear, nleft = _alt_stepwise(A, alt_base[0][5], rollover_schedule(day0))
        out[day0] = (_alt_snapshot(A), lastyear, nleft)
        A.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("day0", [364, 180], ids=["january", "july"])
def test_run_with_rollover_and_irrigation_in_one_pad_word(alt_base, alt_stepwise_result, day0, graph):
    """ELMK_RUN_ALT and ELMK_RUN_IRRIGATION in one run: the step table's pad word holds the rollover bits below the time of day, and
    k_active_layer<true> and k_irrigation<true> each take their part.  Eight half-hour steps across 00:00 of 1 January and across
    00:00 of 1 July, 193 columns on both hemispheres with lat = +0.0 and -0.0 among them, columns whose local 06:00 falls in the
    rollover step (tod 0) and in the steps on either side of it: the run equals the stepwise calls in every field and in the rows of
    the four features.  Not vacuous: ALTMAX_LASTYEAR changed in the hemisphere that rolled, in the rollover step and in no other
    step, and in no column of the other hemisphere; columns checked in the rollover step and hold NLEFT > 0 after it.
    With ELMK_RUN_ALT dropped the irrigation rows are the same (the active layer feeds nothing back).  With ELMK_RUN_IRRIGATION
    dropped the same columns roll; the rows themselves differ, rightly (in 1 of the 193 columns across 1 January and in 3 across
    1 July on an MI355X: the figure is printed), because the applied water changes the soil's heat capacity
    and with it t_soisno - so the other half of the pad word is pinned on a context in which no column is irrigated (sched -1
    throughout): the stage runs and the time of day sits above the rollover bits in every step, nothing is applied, and every field
    and every active-layer row is that of the run without the flag."""
    b, _, sched = alt_base
    north = al.north(b[3])
    steps = rollover_schedule(day0)
    want, lastyear, nleft = alt_stepwise_result[day0]
    B = _alt_context(alt_base, graph)
    B.run(1800.0, steps, ALT_FLAGS)
    got = _alt_snapshot(B)
    _assert_same(got, want, day0)
    B.close()
    rolled = north if day0 == 364 else ~north
    ly0 = _altmax0(NCOL)[1]
    before = np.vstack([ly0[None, :], lastyear[:-1]])
    changed = lastyear.view(np.uint64) != before.view(np.uint64)
    assert changed[ROLL_STEP][rolled].all() and not changed[ROLL_STEP][~rolled].any(), day0
    assert not np.delete(changed, ROLL_STEP, axis=0).any(), day0  # in a step with tod != 0 no column rolled
    assert bits(got["alt"][2][~rolled]) == bits(ly0[~rolled])
    in_roll = (sched >= 0) & (np.arange(NCOL) % 6 == ROLL_STEP - 2)
    assert (nleft[ROLL_STEP][in_roll] == 8.0).any() and (nleft[ROLL_STEP - 1][np.arange(NCOL) % 6 == ROLL_STEP - 3] == 8.0).any()
    assert (nleft[ROLL_STEP + 1][np.arange(NCOL) % 6 == ROLL_STEP - 1] == 8.0).any() and (got["irr"][ir.NLEFT] > 0.0).any()
    # without ELMK_RUN_ALT: the same irrigation rows, and everything else but the active layer's own fields
    P = _alt_context(alt_base, graph, alt=False)
    P.run(1800.0, steps, ALT_FLAGS & ~st.RUN_ALT)
    p = _alt_snapshot(P, alt=False)
    P.close()
    assert bits(p["irr"]) == bits(got["irr"])
    for k in p:
        if k not in ("altmax_indx", "altmax_lastyear_indx"):
            assert same(p[k], got[k]), (day0, k)
    # without ELMK_RUN_IRRIGATION: the same columns roll
    Q = _alt_context(alt_base, graph, irrig=False)
    Q.run(1800.0, steps, ALT_FLAGS & ~st.RUN_IRRIGATION)
    q = _alt_snapshot(Q, irrig=False)
    Q.close()
    print(f"day0={day0}: active-layer rows with and without the irrigation: {int((q['alt'] != got['alt']).any(axis=0).sum())} columns differ")
    assert ((q["alt"][2] != ly0) == (got["alt"][2] != ly0)).all() and ((q["alt"][2] != ly0) == rolled).all()
    # ... and on columns that are not irrigated the flag changes nothing at all
    none = np.full(NCOL, -1, np.int32)
    Z = _alt_context(alt_base, graph, sched=none)
    Z.run(1800.0, steps, ALT_FLAGS)
    z = _alt_snapshot(Z)
    Z.close()
    assert not z["irr"].any()
    del z["irr"]
    _assert_same(z, q, (day0, "no column irrigated"))


# ---- 6. a step that does not divide the day -------------------------------------------------------------------------------------------------
DT7 = 7000.0
NSTEPS7 = 14
NCELL7 = 70
FLAGS7 = st.RUN_IRRIGATION | st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING
PIN_STEP = 11  # (two steps of 7000 s that start a whole day's worth of steps apart share no column's window: 11 is clear of both ends)


def schedule7(nsteps=NSTEPS7):
    """Steps of 7000 s from 23:00 of day 364: the time of day is 82800 + 7000 s reduced mod 86400 - never a multiple of the step -
    and passes midnight in step 1 (into day 0 of the next year) and again in step 13."""
    S = schedule(nsteps)
    for s in range(nsteps):
        sec = (364 * 86400 + 82800 + 7000 * s) % (365 * 86400)
        ddoy = sec / 86400.0
        S[s]["decday"], S[s]["doy"] = ddoy + 1.0, sec // 86400
    assert [int(p["doy"]) for p in S] == [364] + [0] * 12 + [1]
    return S


def tods7(nsteps=NSTEPS7):
    return [(82800 + 7000 * s) % 86400 for s in range(nsteps)]


@pytest.fixture(scope="module")
def base7():
    b = _inputs(NCOL, 531)
    cols = b[0]
    clear_snow(cols)
    rows = prepare(cols, 532)
    c = np.arange(NCOL)
    cols["t_soisno"][:, 5:] = np.maximum(cols["t_soisno"][:, 5:], 276.0)
    tod = np.array(tods7())
    # column c passes 06:00 local in step c % 12 + 1, some seconds before the step's start ...
    sched = ((ir.IRRIG_START - tod[c % 12 + 1] + 500 * (c % 5)) % 86400).astype(np.int32)
    # ... and two kinds pin the time of day of step PIN_STEP to the second: `last` is in by one second there (since = 6999: one second
    # later it would never check), `first` is on the clock's first second (since = 0: one second earlier it would check a step later)
    last, first = c % 12 == 5, c % 12 == 7
    sched[last] = (ir.IRRIG_START + 6999 - tod[PIN_STEP]) % 86400
    sched[first] = (ir.IRRIG_START - tod[PIN_STEP]) % 86400
    sched[c % 7 == 3] = -1
    m = SC.cell_map(NCOL, NCELL7, 71, empty=(0, 63, 64), single=(5,), free=3)
    rng = np.random.default_rng(72)
    down = np.full(NCELL7, -1, np.int32)
    down[1:40] = np.arange(2, 41) % NCELL7
    down[40] = -1
    ddist = np.exp(rng.uniform(np.log(500.0), np.log(60000.0), NCELL7))
    area, _ = SC.cell_values(NCELL7, 73)
    volr0 = 10.0 ** rng.uniform(1.0, 6.0, NCELL7)
    return b, rows, sched, m, down, ddist, area, volr0, (last & (sched >= 0), first & (sched >= 0))


def _context7(base, graph):
    b, rows, sched, m, down, ddist, area, volr0, _ = base
    D = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, NSTEPS7)
    upload_series(D, b[5])
    D.water_balance_enable(TOL)
    D.set_output_grid(*m, fill=NAN)
    D.irrigation_enable(sched)
    D.routing_enable(down, ddist, area, rt.EFFVEL, 2)
    D.routing_set_withdrawal(True)
    D.irrigation_supply_enable(0.1)
    D.routing_init(volr0)
    return D


def _snapshot7(D):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out["hyd"], out["wb"], out["irr"] = D.soil_hydrology_rows(), D.water_balance_rows(), D.irrigation_rows()
    out["route"] = np.stack([D.routing_read(w) for w in range(4)])
    out["sup"] = np.stack([D.irrigation_supply_read(k) for k in SUP])
    return out


@pytest.fixture(scope="module")
def stepwise7(base7):
    A = _context7(base7, False)
    steps = schedule7()
    marked = []
    for s, p in enumerate(steps):
        _physics_inputs(A, base7[0][5], p, DT7)
        A.water_balance_begin()
        st.timestep7_fused(A, DT7)
        tod = ir.time_of_day(float(p["decday"]), int(p["doy"]))
        assert tod == tods7()[s] and tod % 7000 != 0
        A.irrigation(DT7, tod)
        marked.append(A.irrigation_read(ir.NLEFT) == 3.0)
        st.kokkos_soil_temperature(A, DT7)
        st.kokkos_snow_hydrology(A, DT7)
        st.kokkos_surface_fluxes(A, DT7)
        A.soil_hydrology(DT7)
        st.kokkos_evaluate_conservation(A, DT7)
        A.error_summary()
        A.water_balance(DT7)
        A.routing(DT7)
    out = (_snapshot7(A), np.array(marked))
    A.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_at_a_step_that_does_not_divide_the_day(base7, stepwise7, graph):
    """Fourteen steps of 7000 s from 23:00 of 31 December (nspd 3) with the irrigation, the soil hydrology, the water balance, the
    routing and the limit: the time of day is never a multiple of the step and wraps at midnight twice, once across the year's
    end.  The run equals the stepwise calls at irrigation.time_of_day's tod in every field and row.  The rows show the tod the run
    used to the second: the columns whose clock is in by one second in step 11 (since = 6999) check in exactly that step, and the
    columns on the clock's first second there (since = 0) check in that step and not in the next; a tod one second off either way
    would move one of the two kinds."""
    want, marked = stepwise7
    last, first = base7[8]
    B = _context7(base7, graph)
    B.run(DT7, schedule7(), FLAGS7)
    got = _snapshot7(B)
    B.close()
    _assert_same(got, want)
    for kind in (last, first):
        took = marked[:, kind]
        assert took[PIN_STEP].any() and not np.delete(took, PIN_STEP, axis=0)[:, took[PIN_STEP]].any()
        assert not took[:, ~took[PIN_STEP]].any()  # (a column of the kind that is not eligible in step 11 - unstressed, bare - never checks)
        assert (got["irr"][ir.NLEFT][kind][took[PIN_STEP]] == 1.0).all()  # nspd 3, counted down in steps 12 and 13
    assert (got["sup"][ir.UNMET_SUM] > 0.0).any() and marked.any(axis=1).sum() >= 10
