"""Hillslope lateral flow on the device (include/elmk.h "hillslope lateral flow"): k_hillslope_head, k_hillslope_flow<1 | 2 | 4 | 8> and
the hydrology kernel's LAT form against the host restatement (elmkernels_amd/hydrology.py: step with lat=) bit for bit over five chained
steps in both builds, on one column, a chain, stars of every map width and the wide case with its census; the stage inside elmk_run
with the hydrology, water balance and routing flags against the stepwise calls, graph on and off, across a clear and a second enable;
exact restarts through an unchanged image; the clear; tapes; every refusal and both interlocks; the budget; the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics
from elmkernels_amd import hydrology as hy
from elmkernels_amd import regrid as RG
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import hillslope_cases as hc
from tests import river_cases as rv
from tests.hydrology_cases import _new
from tests.river_cases import NSTEPS, river_snapshot
from tests.run_cases import DT, assert_same, same, schedule, stepwise
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

NAN = float("nan")
FLAGS = st.RUN_HYDROLOGY | st.RUN_WATER_BALANCE | st.RUN_ROUTING
ROWS = (rt.VOLR, rt.QIN, rt.QOUT, rt.QOUT_SUM)


def _same_or_nan(got, want):
    """Bit for bit, or NaN on both sides: a NaN stored into a state field is not canonical (the rows' NaNs are)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    eq = (got.view(np.uint8).reshape(got.shape + (got.itemsize,)) == want.view(np.uint8).reshape(want.shape + (want.itemsize,))).all(axis=-1)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    return bool(eq.all())


def _enable(D, G):
    D.hillslope_enable(*hc.lat_of(G))


def _hs_bytes(D, G):
    """What elmk_hillslope_enable allocates: the six rows, the four geometry rows, down, the map, and the reduction's scratch, each
    region rounded up to 256 bytes (the level stride is a multiple of 64, so only the last two round)."""
    ld, npad = D.level_stride, hy.hillslope_map(G["down"]).shape[0]
    up256 = lambda b: (b + 255) // 256 * 256  # noqa: E731
    return up256(6 * 8 * ld) + up256(4 * 8 * ld) + up256(4 * ld) + up256(npad * 4 * ld) + up256(512 * 3 * 8) + 256


# ---- 1. chained steps against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", hc.SHAPES)
def test_five_chained_steps_equal_the_restatement(shape, lib_path):
    """Before every elmk_soil_hydrology the restatement on what the device holds; after it every hydrology row, the six new rows,
    h2osoi_liq / ice / vol and h2osfc bit for bit, every other field untouched, no error bit raised.  The wide case asserts the census
    on what the device held in every step, and the edge columns' values."""
    G = hc.shape(shape)
    cols, scal, soil, rows = hc.columns(G, 21)
    D = _new(cols, scal, soil, rows, lib_path)
    before = D.device_bytes
    _enable(D, G)
    assert D.device_bytes - before > 6 * 8 * D.level_stride
    assert bits(D.hillslope_rows()) == bits(np.zeros((hy.HS_NROWS, G["ncols"])))
    fields = hy.READS + ("h2osoi_vol",)
    for s in range(hc.NSTEPS):
        hit = set()
        want, want_rows, want_hs = hy.step({k: D[k] for k in fields}, D.soil_hydrology_rows(), DT, hit,
                                           stored=np.float32 if lib_path else None, lat=hc.lat_of(G))
        others = {k: D[k] for k in D.fields if k not in hy.WRITES} if s == 0 else {}
        flags = D.error_summary()
        D.soil_hydrology(DT)
        got_rows, got_hs = D.soil_hydrology_rows(), D.hillslope_rows()
        for w in range(hy.HS_NROWS):
            assert bits(got_hs[w]) == bits(want_hs[w]), (s, "hillslope row", w, rv.differing(got_hs[w], want_hs[w]))
        for w in range(hy.NROWS):
            assert bits(got_rows[w]) == bits(want_rows[w]), (s, "row", w, rv.differing(got_rows[w], want_rows[w]))
        for k in hy.WRITES:
            assert _same_or_nan(D[k], want[k]) if shape == "wide" else same(D[k], want[k]), (s, k)
        for k, v in others.items():
            assert same(D[k], v), (s, k)
        assert D.error_summary() == flags
        on = G["down"] != -2
        if shape == "wide":
            assert set(hc.BRANCHES) <= hit, (s, set(hc.BRANCHES) - hit)
            assert np.isnan(got_hs[hy.HS_HEAD, 80]) and np.isnan(got_hs[hy.HS_QLAT_IN, 81]) and got_hs[hy.HS_TRANS, 88] == 0.0
            assert got_hs[hy.HS_QLAT_IN, 256] > 0.0 and got_hs[hy.HS_QLAT_OUT, 255] > 0.0  # across the workgroup boundary
            assert (got_hs[:, ~on] == 0.0).all() and (got_hs[hy.HS_QSTREAM][G["down"] != -1] == 0.0).all()
        elif lib_path is None:
            assert got_hs[hy.HS_QSTREAM, 0] > 0.0 and np.isfinite(got_hs).all()
    part = D.hillslope_read(hy.HS_QLAT_NET, col0=G["ncols"] // 2, n=G["ncols"] - G["ncols"] // 2)
    assert bits(part) == bits(want_hs[hy.HS_QLAT_NET][G["ncols"] // 2:])
    D.close()


def test_all_off_hillslope_and_flat_keep_what_the_statement_says():
    """A context whose columns are all on no hillslope has, after two steps, the bits of a context without the extension in every field
    and row; a flat hillslope moves nothing, and its drainage is the net flux (zero), not F.1's baseflow: a build that wires L3 wrongly
    fails both."""
    G = hc.shape("wide")
    cols, scal, soil, rows = hc.columns(G, 21)
    A, B = _new(cols, scal, soil, rows), _new(cols, scal, soil, rows)
    _enable(A, dict(G, down=np.full(G["ncols"], -2, np.int32)))
    for _ in range(2):
        A.soil_hydrology(DT)
        B.soil_hydrology(DT)
    assert bits(A.soil_hydrology_rows()) == bits(B.soil_hydrology_rows()) and not A.hillslope_rows().any()
    for k in A.fields:
        assert same(A[k], B[k]), k
    assert (B.soil_hydrology_read(hy.QFLX_DRAIN) > 0.0).sum() > 500
    A.close()
    B.close()
    # flat: five equal columns of the wide case's column 60, equal heads, the stream column's head zero
    F = hc.slope5(flat=True)
    F["elev"] = np.full(5, rows[hy.ZWT, 60])
    idx = np.full(5, 60)
    c5 = {k: np.ascontiguousarray(v[idx]) for k, v in cols.items()}
    D = _new(c5, scal, soil, np.ascontiguousarray(rows[:, idx]))
    _enable(D, F)
    D.soil_hydrology(DT)
    hs = D.hillslope_rows()
    assert (hs[hy.HS_HEAD] == 0.0).all() and (hs[hy.HS_TRANS] > 0.0).all() and not hs[hy.HS_QLAT_OUT:].any()
    assert not D.soil_hydrology_read(hy.QFLX_DRAIN).any() and rows[hy.RSUB_TOP_MAX, 60] > 0.0
    D.close()


# ---- 2. the run ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run_base():
    G = rv.run_case()
    G["hs"] = hc.shape("run")
    assert G["hs"]["ncols"] == rv.NCOL
    return G


def _context(G, graph, on=True, lib_path=None):
    D = rv.run_context(G, graph, lib_path, parts=("routing",))
    if on:
        _enable(D, G["hs"])
    return D


def _snapshot(D, hs=True):
    out = river_snapshot(D, ROWS)
    if hs:
        out["hs"] = D.hillslope_rows()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(run_base, graph):
    """Six steps of elmk_run with the three flags and the extension on against the stepwise calls in every field and row; the extension
    cleared between two runs, which drops the captured step and runs the plain form, and enabled again, which brings the launches back."""
    steps = schedule(2 * NSTEPS)
    A, B = _context(run_base, False), _context(run_base, graph)
    stepwise(A, run_base["rec"], steps[:NSTEPS], FLAGS)
    B.run(DT, steps[:NSTEPS], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["hs"][hy.HS_QSTREAM] > 0.0).any() and (a["hs"][hy.HS_QLAT_IN] > 0.0).any() and (a["route"][2] > 0.0).any()
    plain = _context(run_base, False, on=False)
    stepwise(plain, run_base["rec"], steps[:NSTEPS], FLAGS)
    assert not same(plain.soil_hydrology_read(hy.ZWT), a["hyd"][hy.ZWT])  # (the extension does something)
    plain.close()
    for X in (A, B):
        X.hillslope_clear()
    stepwise(A, run_base["rec"], steps[NSTEPS:NSTEPS + 2], FLAGS)
    B.run(DT, steps[NSTEPS:NSTEPS + 2], FLAGS)
    assert_same(_snapshot(B, False), _snapshot(A, False))
    for X in (A, B):
        _enable(X, run_base["hs"])
    stepwise(A, run_base["rec"], steps[NSTEPS + 2:NSTEPS + 4], FLAGS)
    B.run(DT, steps[NSTEPS + 2:NSTEPS + 4], FLAGS)
    a = _snapshot(A)
    assert_same(_snapshot(B), a)
    assert (a["hs"][hy.HS_QSTREAM] > 0.0).any() and B.routing_count() == NSTEPS + 4
    A.close()
    B.close()


def test_restart_3_plus_3_equals_6(run_base):
    """Three steps, an image, a fresh context with the extension enabled by the driver, three more: the bits of six steps in one
    context.  The image has the size of the image of a context without the extension."""
    steps = schedule(NSTEPS)
    A = _context(run_base, True)
    A.run(DT, steps, FLAGS)
    want = _snapshot(A)
    A.close()
    P = _context(run_base, True, on=False)
    size_plain = P.restart_size()
    P.close()
    B = _context(run_base, True)
    assert B.restart_size() == size_plain
    B.run(DT, steps[:3], FLAGS)
    img, volr, qsum, count = B.restart_save(), B.routing_read(rt.VOLR), B.routing_read(rt.QOUT_SUM), B.routing_count()
    assert img.size == size_plain
    B.close()
    Cx = _context(run_base, True)
    Cx.restart_load(img)
    Cx.routing_init(volr, qsum, count)
    Cx.run(DT, steps[3:], FLAGS)
    assert_same(_snapshot(Cx), want)
    Cx.close()


def test_clear_returns_to_the_plain_stage(run_base):
    """Two steps with the extension, the clear, and a context that never had it given the same fields and rows: two more steps give the
    same bits everywhere, and the bytes of the extension are returned."""
    A, B = _context(run_base, False), _context(run_base, False, on=False)
    bytes_b, size_b = B.device_bytes, B.restart_size()
    assert A.device_bytes - bytes_b == _hs_bytes(A, run_base["hs"]) and A.restart_size() == size_b
    steps = schedule(4)
    stepwise(A, run_base["rec"], steps[:2], FLAGS)
    assert (A.hillslope_read(hy.HS_QSTREAM) > 0.0).any()
    A.hillslope_clear()
    A.hillslope_clear()  # nothing to free: OK
    assert A.device_bytes == bytes_b and A.restart_size() == size_b
    with pytest.raises(L.ElmkError, match=r"not enabled \(elmk_hillslope_enable\)"):
        A.hillslope_read(hy.HS_HEAD)
    for k in A.fields:
        B[k] = A[k]
    hrows = A.soil_hydrology_rows()
    B.soil_hydrology_init(hrows[hy.ZWT], hrows[hy.WA])
    volr = A.routing_read(rt.VOLR)
    for X in (A, B):  # (the same call on both: an init zero-fills the diagnostics and the mean)
        X.routing_init(volr)
    stepwise(A, run_base["rec"], steps[2:], FLAGS)
    stepwise(B, run_base["rec"], steps[2:], FLAGS)
    assert_same(_snapshot(A, False), _snapshot(B, False))
    A.close()
    B.close()


# ---- 3. tapes ------------------------------------------------------------------------------------------------------------------------------
def _fold(samples, op):
    acc = None
    for v in samples:
        if op == "avg":
            acc = (-0.0 + v) if acc is None else acc + v
        else:
            a = np.full(v.shape, -np.inf) if acc is None else acc
            acc = np.where((v > a) | np.isnan(v), v, a)
    return acc / float(len(samples)) if op == "avg" else acc


def test_rows_on_history_tapes(run_base):
    """A column entry (AVG, MAX) and a gridded entry (AVG) on QLAT_NET equal the numpy folds of the row read after each step; a point
    series entry takes the row; while an entry exists the clear is refused and changes nothing."""
    D = _context(run_base, False)
    col = {op: D.history_add_row(0, "hillslope", hy.HS_QLAT_NET, op) for op in ("avg", "max")}
    cell = D.gridded_history_add_row(0, "hillslope", hy.HS_QLAT_NET, "avg")
    samples = []
    stepwise(D, run_base["rec"], schedule(3), FLAGS | st.RUN_HISTORY, per_step=(samples, lambda X: X.hillslope_read(hy.HS_QLAT_NET)))
    assert bits(samples[0]) != bits(samples[-1]) and (np.array(samples) != 0.0).any()
    for op, e in col.items():
        assert bits(D.history_read(e)) == bits(_fold(samples, op)), op
    ptr, cidx, w = run_base["map"]
    want = _fold([RG.apply_aggregate(ptr, cidx, w, s, NAN) for s in samples], "avg")
    got = D.history_read(cell)
    empty = np.diff(ptr) == 0
    assert got.shape == (rv.NCELL,) and np.isnan(got[empty]).all() and bits(got[~empty]) == bits(want[~empty])
    state, nbytes = _snapshot(D), D.device_bytes
    with pytest.raises(L.ElmkError, match="elmk_hillslope_clear: history entries over the hillslope rows exist \\(elmk_history_clear first\\)"):
        D.hillslope_clear()
    assert D.device_bytes == nbytes
    assert_same(_snapshot(D), state)
    D.history_clear()
    for call in (lambda: D.history_add_row(0, "hillslope", hy.HS_NROWS, "avg"), lambda: D.history_add_row(0, "hillslope", -1, "avg")):
        with pytest.raises(L.ElmkError, match="unknown row"):
            call()
    D.points_set("columns", [0, 5, 100])
    e = D.points_add_row("hillslope", hy.HS_QLAT_NET)
    D.points_reserve(4)
    D.points_record(1.0)
    assert bits(D.points_read(e)[0]) == bits(samples[-1][[0, 5, 100]])
    with pytest.raises(L.ElmkError, match="elmk_points_clear first"):
        D.hillslope_clear()
    D.points_clear()
    D.hillslope_clear()
    with pytest.raises(L.ElmkError, match="not enabled"):
        D.history_add_row(0, "hillslope", hy.HS_QLAT_NET, "avg")
    D.close()


# ---- 4. refusals and interlocks ------------------------------------------------------------------------------------------------------------
def test_refusals_and_interlocks_change_nothing(run_base):
    G = run_base
    H = G["hs"]
    n = H["ncols"]

    def refused(call, match):
        with pytest.raises(L.ElmkError, match=match):
            call()

    from tests import helpers
    b = G["b"]
    D = helpers.device_state(b[0], b[1], b[2], lat=b[3], lon=b[4])
    refused(lambda: _enable(D, H), "elmk_hillslope_enable: the soil hydrology is not enabled")
    refused(lambda: D.hillslope_read(0), r"elmk_hillslope_read: not enabled \(elmk_hillslope_enable\)")
    refused(D.hillslope_budget, "elmk_hillslope_budget: not enabled")
    D.hillslope_clear()  # nothing to free: OK
    D.close()

    D = _context(G, False, on=False)
    bytes0, size0, state0 = D.device_bytes, D.restart_size(), _snapshot(D, False)
    vec = lambda a, i, v: np.where(np.arange(n) == i, v, a)  # noqa: E731
    on = int(np.nonzero(H["down"] != -2)[0][3])
    off = int(np.nonzero(H["down"] == -2)[0][0])
    feeder = int(np.nonzero(H["down"] >= 0)[0][0])
    top = feeder  # the stream column of feeder's hillslope: drained into feeder, it closes a cycle
    while H["down"][top] >= 0:
        top = int(H["down"][top])
    en = lambda **kw: (lambda: D.hillslope_enable(*hc.lat_of(dict(H, **kw))))  # noqa: E731
    for call, match in ((en(down=vec(H["down"], on, -3)), f"down outside .* at column {on}"), (en(down=vec(H["down"], on, n)), f"down outside .* at column {on}"),
                        (en(down=vec(H["down"], on, on)), f"down equals its own index at column {on}"),
                        (en(down=vec(H["down"], feeder, off)), f"down names a column on no hillslope at column {feeder}"),
                        (en(down=np.where(np.arange(n) < 10, np.array([-1] + [0] * (n - 1)), H["down"]).astype(np.int32)), "more than 8 uphill columns .* at column 9"),
                        (en(down=vec(H["down"], top, feeder)), "the hillslope has a cycle at column"),
                        (en(dist=vec(H["dist"], on, 0.0)), f"dist not finite and > 0 at column {on}"), (en(width=vec(H["width"], on, NAN)), f"width not finite and > 0 at column {on}"),
                        (en(area=vec(H["area"], on, -1.0)), f"area not finite and > 0 at column {on}"), (en(elev=vec(H["elev"], on, np.inf)), f"elev not finite at column {on}"),
                        (en(k_aniso=0.0), "k_aniso not finite and > 0$"), (en(k_aniso=NAN), "k_aniso not finite and > 0$")):
        refused(call, "elmk_hillslope_enable: " + match)
    P = C.c_void_p
    arrs = [np.ascontiguousarray(H["down"], np.int32)] + [np.ascontiguousarray(H[k], np.float64) for k in ("dist", "width", "area", "elev")]
    ptrs = [a.ctypes.data_as(P) for a in arrs]
    for k in range(5):
        args = list(ptrs)
        args[k] = None
        assert D.lib.elmk_hillslope_enable(D.ctx, *args, 50.0) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    with captured(D) as cap:
        rc = D.lib.elmk_hillslope_enable(D.ctx, *ptrs, 50.0)
        cap.end()
        assert rc == -1 and b"captured" in D.lib.elmk_last_error(D.ctx)
    assert D.device_bytes == bytes0 and D.restart_size() == size0
    assert_same(_snapshot(D, False), state0)
    # the interlocks, one direction: the other extension on refuses the enable and names its clear
    D.soil_hydrology_frost_enable(1.0e-6)
    bytes_f = D.device_bytes
    refused(lambda: _enable(D, H), r"elmk_hillslope_enable: the frost table is on \(elmk_soil_hydrology_frost_clear first\)")
    assert D.device_bytes == bytes_f
    D.soil_hydrology_frost_clear()
    _enable(D, H)
    bytes1 = D.device_bytes
    assert bytes1 - bytes0 == _hs_bytes(D, H) and D.restart_size() == size0
    S2 = schedule(2)
    stepwise(D, G["rec"], S2[:1], FLAGS)
    state1 = _snapshot(D)
    # ... and the other direction
    refused(lambda: _enable(D, H), "elmk_hillslope_enable: already on")
    refused(lambda: D.soil_hydrology_frost_enable(1.0e-6), r"elmk_soil_hydrology_frost_enable: the hillslope lateral flow is on \(elmk_hillslope_clear first\)")
    for call, match in ((lambda: D.hillslope_read(hy.HS_NROWS), "unknown row"), (lambda: D.hillslope_read(-1), "unknown row"),
                        (lambda: D.hillslope_read(0, col0=n, n=1), "column range"), (lambda: D.hillslope_read(0, col0=n - 1, n=2), "column range")):
        refused(call, match)
    assert D.lib.elmk_hillslope_budget(D.ctx, None) == -1 and b"null argument" in D.lib.elmk_last_error(D.ctx)
    buf = np.zeros(n)
    with captured(D) as cap:
        rcs = (D.lib.elmk_hillslope_clear(D.ctx), D.lib.elmk_hillslope_budget(D.ctx, buf.ctypes.data_as(P)),
               D.lib.elmk_hillslope_read(D.ctx, 0, buf.ctypes.data_as(P), 0, n))
        cap.end()
        assert rcs == (-1, -1, -1)
    assert D.device_bytes == bytes1
    assert_same(_snapshot(D), state1)
    # the following step is the step of a context that met no refusal
    W = _context(G, False)
    stepwise(W, G["rec"], S2, FLAGS)
    stepwise(D, G["rec"], S2[1:], FLAGS)
    assert_same(_snapshot(D), _snapshot(W))
    W.close()
    D.routing_clear()
    D.soil_hydrology_clear()  # frees the extension too
    refused(lambda: D.hillslope_read(0), "not enabled")
    D.close()


def test_the_floodplain_infiltration_interlock():
    """Both directions against the floodplain infiltration: each enable is refused while the other is on and names the other's clear."""
    from tests import floodplain_infiltration_cases as fc

    G = fc.run_case()
    H = hc.shape("run")
    H = dict(H, **{k: np.resize(H[k], G["ncols"]) for k in ("dist", "width", "area", "elev")}, down=np.full(G["ncols"], -1, np.int32), ncols=G["ncols"])
    D = _new(G["cols"], G["scal"], G["soil"], G["rows"], None, G["lat"], G["lon"])
    D.water_balance_enable(rv.TOL)
    D.set_output_grid(*G["map"], fill=NAN)
    D.routing_enable(G["down"], G["ddist"], G["area"], rt.EFFVEL, fc.NSUB)
    D.routing_kinematic_enable(G["p"])
    D.routing_inundation_enable(G["rdepth"], G["eprof"])
    D.floodplain_infiltration_enable()
    nbytes = D.device_bytes
    with pytest.raises(L.ElmkError, match=r"elmk_hillslope_enable: the floodplain infiltration is on \(elmk_floodplain_infiltration_clear first\)"):
        _enable(D, H)
    assert D.device_bytes == nbytes
    D.floodplain_infiltration_clear()
    _enable(D, H)
    nbytes = D.device_bytes
    with pytest.raises(L.ElmkError, match=r"elmk_floodplain_infiltration_enable: the hillslope lateral flow is on \(elmk_hillslope_clear first\)"):
        D.floodplain_infiltration_enable()
    assert D.device_bytes == nbytes
    D.hillslope_clear()
    D.floodplain_infiltration_enable()
    D.close()


# ---- 5. the budget -------------------------------------------------------------------------------------------------------------------------
def test_budget_equals_the_reduction():
    """elmk_hillslope_budget against diagnostics.reduce_min_max_sum of the QSTREAM row, bit for bit; the call changes no row."""
    G = hc.shape("wide")
    cols, scal, soil, rows = hc.columns(G, 21)
    for k, v in hc.W_EDGE_ZWT.items():
        rows[hy.ZWT, k] = 2.0 if not np.isfinite(v) else v
    D = _new(cols, scal, soil, rows)
    _enable(D, G)
    assert bits(D.hillslope_budget()) == bits(np.zeros(1))
    D.soil_hydrology(DT)
    hs = D.hillslope_rows()
    want = np.array([diagnostics.reduce_min_max_sum(hs[hy.HS_QSTREAM])[2]])
    assert np.isfinite(want).all() and want[0] > 0.0 and bits(want) == bits(hy.hillslope_budget(hs[hy.HS_QSTREAM]))
    for _ in range(2):
        assert bits(D.hillslope_budget()) == bits(want)
    assert bits(D.hillslope_rows()) == bits(hs)
    # elmk_soil_hydrology_clear frees the extension too, unless an entry reads its rows
    D.history_add_row(0, "hillslope", hy.HS_QSTREAM, "avg")
    nbytes = D.device_bytes
    with pytest.raises(L.ElmkError, match="elmk_soil_hydrology_clear: history entries over the hillslope rows exist \\(elmk_history_clear first\\)"):
        D.soil_hydrology_clear()
    assert D.device_bytes == nbytes and bits(D.hillslope_rows()) == bits(hs)
    D.history_clear()
    D.soil_hydrology_clear()
    with pytest.raises(L.ElmkError, match="not enabled"):
        D.hillslope_read(hy.HS_HEAD)
    D.close()


# ---- the example ---------------------------------------------------------------------------------------------------------------------------
def test_hillslope_demo(tmp_path):
    """examples/hillslope_demo.cc builds with g++ against the C ABI and runs: 96 steps with and without the extension; the toe ends
    wetter than the ridge with it, they end equal without it, and the stream discharges in every step."""
    out = run_demo(build_demo("hillslope_demo", tmp_path), timeout=120).stdout.splitlines()
    steps = [s.split() for s in out if s.split() and s.split()[0].isdigit()]
    assert [int(s[0]) for s in steps] == list(range(96)) and "hillslope lateral flow, 96 steps" in out[0]
    ridge, toe, q, ridge_off, toe_off = (np.array([float(s[k]) for s in steps]) for k in (1, 2, 3, 4, 5))
    assert toe[-1] < ridge[-1] and (ridge_off == toe_off).all() and (q > 0.0).all() and np.isfinite(np.array([ridge, toe, q])).all()


# ---- the cost tool -------------------------------------------------------------------------------------------------------------------------
def test_cost_tool_every_mode_at_the_smallest_size(tmp_path):
    """tests/tools/cost_hillslope.py, every mode, once at 4096 columns, two rounds, two run steps, a copy of the library standing in for
    the parent's and for its second copy: the records hold every mode's timings, finite and positive, the stream discharges where
    there is a stream, and every context is closed again.  Timings are not compared at this size."""
    import json
    import math
    import os
    import shutil
    import sys

    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import cost_hillslope as CH

    live = set()
    create, close = st.ELMState.__init__, st.ELMState.close

    def counted_create(self, *a, **kw):
        create(self, *a, **kw)
        live.add(id(self))

    def counted_close(self):
        close(self)
        live.discard(id(self))

    st.ELMState.__init__, st.ELMState.close = counted_create, counted_close
    try:
        lib, lib2 = (shutil.copy(L.LIB_PATH, str(tmp_path / name)) for name in ("libelmk_other.so", "libelmk_other2.so"))
        recs = {"measure": CH.measure(4096, 2), "run": CH.measure_run(4096, 2, 2), "parent": CH.parent_off(4096, 2, 2, lib, False),
                "parent_first_parent2": CH.parent_off(4096, 2, 2, lib, True, lib2)}
    finally:
        st.ELMState.__init__, st.ELMState.close = create, close
    assert not live, f"{len(live)} contexts left open"
    recs = json.loads(json.dumps(recs))
    m = recs["measure"]
    assert set(m["ms_all"]) == {"hyd_plain", "hyd_lat_off", "hyd_lat_chain5", "hyd_lat_star8", "accum_t10"}
    assert all(len(v) == 2 and all(math.isfinite(x) and x > 0.0 for x in v) for v in m["ms_all"].values())
    assert m["stream_discharge_m3s"]["hyd_lat_off"] == 0.0 and m["stream_discharge_m3s"]["hyd_lat_chain5"] > 0.0
    assert m["stream_discharge_m3s"]["hyd_lat_star8"] > 0.0 and set(m["added_ms"]) == set(CH.SHAPES) == set(m["added_bytes_per_column"])
    assert m["added_bytes_per_column"]["chain5"]["head"] == 53 * 8 + 4 + 16 and m["plain_TBps"] > 0.0 and m["accum_t10_GBps"] > 0.0
    r = recs["run"]
    assert set(r["ms_all"]) == {"run+hyd", "run+hyd+lat"} and all(x > 0.0 for v in r["ms_all"].values() for x in v)
    for label, first in (("parent", "this"), ("parent_first_parent2", "parent")):
        p = recs[label]
        assert p["first_context"] == first and set(p["ms_all"]) == {"this", "parent"} and set(p["this_over_parent"]) == {"run_step", "hydrology"}
        assert all(len(v) == 2 and all(x > 0.0 for x in v) for d in p["ms_all"].values() for v in d.values())
    assert recs["parent_first_parent2"]["this"] == "libelmk_other2.so" and recs["parent"]["this"] == "libelmk.so"
