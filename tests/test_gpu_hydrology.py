"""Soil hydrology on the device (include/elmk.h "soil hydrology"): k_soil_hydrology against the host restatement
(elmkernels_amd/hydrology.py: step) bit for bit in both builds, on generated columns that take every branch; a six-step chain through
the physics; the stage inside elmk_run against the stepwise calls, graph on and off; exact restarts; every refusal; no effect on a
context without the feature; and the closure of the water budget against the host chain."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests.parity_cases import WETLAND
from tests.hydrology_cases import (BRANCHES, CHAIN_STEPS, CLOSURE_BOUND, CLOSURE_FIELDS, CLOSURE_MEASURED, _new, _physics, clear_snow,
                                   closure, generated, host_chain, prepare)
from tests.run_cases import DT, NREC, SERIES, _inputs, device, same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, run_demo

pytestmark = pytest.mark.gpu

STEP_FIELDS = hy.READS + ("h2osoi_vol",)


def _host_step(D, hit=None, lib_path=None):
    """hydrology.step on what the device holds (fp32 as stored in the fp32-state build) -> the fields and rows it must hold afterwards."""
    return hy.step({k: D[k] for k in STEP_FIELDS}, D.soil_hydrology_rows(), DT, hit, stored=np.float32 if lib_path else None)


def _assert_step(D, others, want, want_rows, what=""):
    got_rows = D.soil_hydrology_rows()
    for w in range(hy.NROWS):
        assert bits(got_rows[w]) == bits(want_rows[w]), (what, "row", w)
    for k in hy.WRITES:
        assert same(D[k], want[k]), (what, k)
    for k, v in others.items():
        assert same(D[k], v), (what, k)


@pytest.mark.parametrize("n", [1001, 4700])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_one_step_equals_the_restatement(n, lib_path):
    """Ragged against 256-lane workgroups.  Every written field and every row of the feature against hydrology.step, every other
    field untouched; the host restatement says that every branch of the stage was taken."""
    cols, scal, soil, rows = generated(n, 300 + n, full=True)
    D = _new(cols, scal, soil, rows, lib_path)
    assert D.level_stride != n
    assert bits(D.soil_hydrology_rows()[:hy.QFLX_SURF]) == bits(rows[:hy.QFLX_SURF])
    hit = set()
    want, want_rows = _host_step(D, hit, lib_path)
    assert hit == BRANCHES, BRANCHES - hit
    others = {k: D[k] for k in D.fields if k not in hy.WRITES}
    D.soil_hydrology(DT)
    _assert_step(D, others, want, want_rows)
    part = D.soil_hydrology_read(hy.ZWT, col0=n // 2, n=n - n // 2)
    assert bits(part) == bits(want_rows[hy.ZWT][n // 2:])
    D.close()


def test_cold_start():
    """NULL for zwt and wa: wa = 4000 mm and zwt from the column's zisoi, as hydrology.cold_start_zwt has it; both builds."""
    cols, scal, soil, rows = generated(193, 8, full=True)
    for lib_path in (None, L.F32_LIB_PATH):
        D = _new(cols, scal, soil, rows, lib_path)
        D.soil_hydrology_init()
        zi9 = D["zisoi"][:, hy.NLEVSNO + hy.N].astype(np.float64)
        want = np.array([hy.cold_start_zwt(float(v)) for v in zi9])
        assert bits(D.soil_hydrology_read(hy.ZWT)) == bits(want) and bits(D.soil_hydrology_read(hy.WA)) == bits(np.full(193, 4000.0))
        assert np.all(np.abs(want - (zi9 + 5.0)) < 1e-12)
        D.close()


# ---- the chain --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_inputs():
    return generated(1001, 77, full=True, chain=True)


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_six_step_chain_equals_the_restatement(chain_inputs, lib_path):
    """elmk_advance_physics, then the stage, six times: after every stage the device against hydrology.step on what the device held
    before it."""
    cols, scal, soil, rows = chain_inputs
    D = _new(cols, scal, soil, rows, lib_path)
    hit = set()
    for s in range(CHAIN_STEPS):
        _physics(D)
        want, want_rows = _host_step(D, hit, lib_path)
        others = {k: D[k] for k in D.fields if k not in hy.WRITES}
        D.soil_hydrology(DT)
        _assert_step(D, others, want, want_rows, s)
    assert {"jwt_mid", "jwt_N", "table_rises", "table_falls", "drain_soil", "drain_aquifer", "snl_0", "snl_pos", "imped"} <= hit
    D.close()


def test_closure_of_the_water_budget(chain_inputs):
    """errh2o of the closed budget (hydrology.water_balance_error from downloads) on the snow-free columns without surface water of
    the six-step chain: bit-equal to the same quantity of the host chain (the oracle's step plus hydrology.step), under CLOSURE_BOUND
    = 10 x CLOSURE_MEASURED (0.9000328415202219 mm, measured on the host chain), on more than half of the columns; a context without
    the stage leaves (rain - evaporation) * dt there."""
    cols, scal, soil, rows = chain_inputs
    _, _, host = host_chain(cols, scal, soil, rows)
    D = _new(cols, scal, soil, rows)
    P = device((cols, scal, soil, *synth.global_grid(rows.shape[1], seed=9)))
    assert CLOSURE_BOUND == 10.0 * CLOSURE_MEASURED
    for s in range(CHAIN_STEPS):
        wa_beg = D.soil_hydrology_read(hy.WA)
        st.kokkos_init_timestep(D)
        sno_beg = D["h2osno"]
        st.advance_physics(D, DT)
        D.soil_hydrology(DT)
        e, keep = closure({k: D[k] for k in CLOSURE_FIELDS}, wa_beg, sno_beg, D.soil_hydrology_rows(), DT)
        he, hkeep = host[s]
        assert np.array_equal(keep, hkeep) and keep.mean() > 0.5, s
        print(f"step {s}: kept {keep.mean():.3f}, max |errh2o| {np.abs(e[keep]).max():.17g}, median {np.median(np.abs(e[keep])):.3e}")
        assert bits(e[keep]) == bits(he[keep]), s
        assert np.abs(e[keep]).max() < CLOSURE_BOUND
        st.kokkos_init_timestep(P)
        sno_beg = P["h2osno"]
        st.advance_physics(P, DT)
        e0, keep0 = closure({k: P[k] for k in CLOSURE_FIELDS}, wa_beg, sno_beg, None, DT, with_stage=False)
        assert keep0.mean() > 0.5
        assert np.median(np.abs(e0[keep0])) > 1.0e-3 > 1.0e-9 > np.median(np.abs(e[keep])), s
    D.close()
    P.close()


# ---- the run ----------------------------------------------------------------------------------------------------------------------
NCOL = 200
NSTEPS = 4


@pytest.fixture(scope="module")
def base():
    b = _inputs(NCOL, 431)
    clear_snow(b[0])
    rows = prepare(b[0], 432)
    return b, rows


def _context(base, graph, lib_path=None, enable=True):
    b, rows = base
    D = _new(b[0], b[1], b[2], rows, lib_path, b[3], b[4]) if enable else device(b, lib_path=lib_path)
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    return D


def _snapshot(D, rows=True):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    if rows:
        out["rows"] = D.soil_hydrology_rows()
    return out


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for k, v in a.items():
        assert same(v, b[k]), k


@pytest.fixture(scope="module")
def stepwise_result(base):
    A = _context(base, False)
    diag = stepwise(A, base[0][5], schedule(NSTEPS), st.RUN_HYDROLOGY)
    out = (diag, _snapshot(A))
    A.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_run_equals_stepwise(base, stepwise_result, graph):
    """elmk_run with ELMK_RUN_HYDROLOGY over four steps against the stepwise calls with elmk_soil_hydrology between
    elmk_advance_physics and the conservation row: the diagnostics rows, every state field and every row of the feature.  Graph on and
    graph off therefore give the same bits."""
    want_diag, want = stepwise_result
    B = _context(base, graph)
    B.run(DT, schedule(NSTEPS), st.RUN_HYDROLOGY)
    for g, w in zip(B.run_diagnostics(), want_diag):
        assert same(g, w)
    got = _snapshot(B)
    _assert_same(got, want)
    assert not bits(got["rows"][hy.ZWT]) == bits(base[1][hy.ZWT]) and np.isfinite(got["rows"]).all()
    B.close()


def test_restart_n_plus_n_equals_2n(base):
    """Two steps, a version-4 image, a fresh context with the feature, two more steps: the bits of four steps in one context.  The
    image holds ZWT and WA last; it is refused by a context without the feature, and a version-1 image by one with it."""
    S4 = schedule(NSTEPS)
    A = _context(base, True)
    A.run(DT, S4, st.RUN_HYDROLOGY)
    want = _snapshot(A)
    A.close()
    B = _context(base, True)
    B.run(DT, S4[:2], st.RUN_HYDROLOGY)
    img = B.restart_save()
    assert img.size == B.restart_size()
    p = R.verify(img)
    assert int(p["header"]["version"]) == R.VERSION_HYDROLOGY == 4
    assert [(int(s["kind"]), int(s["id"])) for s in p["sections"][-2:]] == [(R.HYDROLOGY_SECTION, hy.ZWT), (R.HYDROLOGY_SECTION, hy.WA)]
    assert bits(p["data"][-2]) == bits(B.soil_hydrology_read(hy.ZWT)) and bits(p["data"][-1]) == bits(B.soil_hydrology_read(hy.WA))
    B.close()
    b, rows = base
    C = _new(b[0], b[1], b[2], np.where(np.arange(hy.NROWS)[:, None] < 2, 1.0, rows), None, b[3], b[4])  # other ZWT and WA: the image's win
    C.set_graph(True)
    C.run_reserve(NREC, 2 * NSTEPS)
    upload_series(C, b[5])
    C.restart_load(img)
    C.run(DT, S4[2:], st.RUN_HYDROLOGY)
    _assert_same(_snapshot(C), want)
    # the features of image and context must match
    plain = _context(base, True, enable=False)
    old = plain.restart_save()
    assert int(R.verify(old)["header"]["version"]) == 1
    before = _snapshot(plain, rows=False)
    with pytest.raises(L.ElmkError):
        plain.restart_load(img)
    _assert_same(_snapshot(plain, rows=False), before)
    before = _snapshot(C)
    with pytest.raises(L.ElmkError):
        C.restart_load(old)
    _assert_same(_snapshot(C), before)
    plain.close()
    C.close()


def test_refusals_change_nothing(base):
    b, rows = base
    D = _context(base, True, enable=False)
    S1 = schedule(1)
    size0, bytes0 = D.restart_size(), D.device_bytes
    before = _snapshot(D, rows=False)
    for call in (lambda: D.soil_hydrology(DT), lambda: D.soil_hydrology_init(), lambda: D.soil_hydrology_read(hy.ZWT),
                 lambda: D.soil_hydrology_set_params(rows[hy.HKSAT:hy.HKSAT + hy.N], 0.1, 1.0, 0.1, 0.1),
                 lambda: D.run(DT, S1, st.RUN_HYDROLOGY)):  # not enabled
        with pytest.raises(L.ElmkError):
            call()
    D.soil_hydrology_clear()  # nothing to free: OK
    assert D.restart_size() == size0 and D.device_bytes == bytes0
    D.soil_hydrology_enable()
    size1, bytes1 = D.restart_size(), D.device_bytes
    assert bytes1 - bytes0 == hy.NROWS * 8 * D.level_stride and size1 > size0
    with pytest.raises(L.ElmkError):  # twice
        D.soil_hydrology_enable()
    for call in (lambda: D.soil_hydrology(DT), lambda: D.run(DT, S1, st.RUN_HYDROLOGY)):  # parameters never set
        with pytest.raises(L.ElmkError):
            call()
    D.soil_hydrology_set_params(rows[hy.HKSAT:hy.HKSAT + hy.N], rows[hy.WTFACT], rows[hy.H2OSFC_THRESH], rows[hy.K_WET], rows[hy.RSUB_TOP_MAX])
    D.soil_hydrology_init(rows[hy.ZWT], rows[hy.WA])
    r0 = D.soil_hydrology_rows()
    for dt in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.ElmkError):
            D.soil_hydrology(dt)
    for call in (lambda: D.soil_hydrology_read(hy.NROWS), lambda: D.soil_hydrology_read(-1), lambda: D.soil_hydrology_read(hy.ZWT, col0=NCOL, n=1)):
        with pytest.raises(L.ElmkError):
            call()
    assert bits(D.soil_hydrology_rows()) == bits(r0) and D.restart_size() == size1 and D.device_bytes == bytes1
    _assert_same(_snapshot(D, rows=False), before)
    # a land unit that is not soil or crop: nothing is enqueued, OK
    D.set_land(**dict(synth.TEST_LAND, ltype=4))
    D.soil_hydrology(DT)
    assert bits(D.soil_hydrology_rows()) == bits(r0)
    _assert_same(_snapshot(D, rows=False), before)
    D.soil_hydrology_clear()
    assert D.restart_size() == size0 and D.device_bytes == bytes0
    D.close()


def test_a_context_without_the_feature_is_what_it_was(base):
    """A never touches the feature.  B enables it, sets parameters, runs flagged steps and clears it; then its state is put back and it
    runs what A runs.  C keeps the feature enabled and live beside them and runs unflagged.  All three: the bits of the stepwise calls
    of the parent behaviour in every state field and diagnostics row; A and the cleared B: the same device bytes and the same
    version-1 image, byte for byte; the feature's rows of C untouched by an unflagged run."""
    b, rows = base
    S4 = schedule(NSTEPS)
    A = _context(base, True, enable=False)
    bytes0, size0 = A.device_bytes, A.restart_size()
    image0 = A.restart_save()
    assert int(R.verify(image0)["header"]["version"]) == 1
    # B: a life with the feature, on this graph slot, then back to where A starts
    B = _context(base, True)
    B.run(DT, S4, st.RUN_HYDROLOGY)
    assert B.device_bytes > bytes0 and B.restart_size() > size0
    B.soil_hydrology_clear()
    assert B.device_bytes == bytes0 and B.restart_size() == size0
    for k, v in b[0].items():
        B.upload(k, v)
    # C: the feature enabled and initialised, never flagged
    C = _context(base, True)
    rows_c = C.soil_hydrology_rows()
    # the parent behaviour: the stepwise calls, graph off
    P = _context(base, False, enable=False)
    want_diag = stepwise(P, b[5], S4)
    want = _snapshot(P, rows=False)
    P.close()
    for D in (A, B, C):
        D.run(DT, S4, 0)
        for g, w in zip(D.run_diagnostics(), want_diag):
            assert same(g, w)
        _assert_same(_snapshot(D, rows=False), want)
    ia, ib = A.restart_save(), B.restart_save()
    pa, pb = R.verify(ia), R.verify(ib)
    differ = [(int(x["kind"]), int(x["id"])) for x, da, db in zip(pa["sections"], pa["data"], pb["data"]) if bits(da) != bits(db)]
    assert not differ, differ
    assert bits(ia) == bits(ib) and int(pa["header"]["version"]) == 1 and ia.size == size0
    assert A.device_bytes == bytes0 and B.device_bytes == bytes0
    assert bits(C.soil_hydrology_rows()) == bits(rows_c)
    # and a flagged run after an unflagged one on the same context takes the stage in again (the captured step follows the flag)
    C.run(DT, S4[:1], st.RUN_HYDROLOGY)
    assert bits(C.soil_hydrology_rows()) != bits(rows_c)
    for D in (A, B, C):
        D.close()


def test_the_captured_run_step_follows_the_land_unit(base):
    """The stage is in the run step only where the land unit is soil or crop.  A flagged run captures its step; after elmk_set_land to
    another land unit the same flagged run leaves the feature's rows and the soil water to the rest of the physics, and back on soil
    it runs the stage again - with the graph as without it."""
    S1 = schedule(1)
    got = {}
    for graph in (True, False):
        D = _context(base, graph)
        D.run(DT, S1, st.RUN_HYDROLOGY)
        r1 = D.soil_hydrology_rows()
        assert bits(r1[hy.ZWT]) != bits(base[1][hy.ZWT])
        D.set_land(**WETLAND)
        D.run(DT, S1, st.RUN_HYDROLOGY)
        assert bits(D.soil_hydrology_rows()) == bits(r1), graph
        D.set_land(**synth.TEST_LAND)
        D.run(DT, S1, st.RUN_HYDROLOGY)
        r3 = D.soil_hydrology_rows()
        assert bits(r3[hy.ZWT]) != bits(r1[hy.ZWT]), graph
        got[graph] = _snapshot(D)
        D.close()
    _assert_same(got[True], got[False])


def test_restart_says_which_feature_differs(base):
    """A version-4 image with the active layer rows against a context with the soil hydrology alone, and the other way round: refused
    with a message that names the feature, nothing changed."""
    both = _context(base, True)
    both.active_layer_enable()
    only = _context(base, True)
    for src, dst, word in ((both, only, "not enabled"), (only, both, "holds no such rows")):
        img = src.restart_save()
        assert int(R.verify(img)["header"]["version"]) == 4
        before = _snapshot(dst)
        with pytest.raises(L.ElmkError, match="active layer.*" + word + "|" + word + ".*active layer"):
            dst.restart_load(img)
        _assert_same(_snapshot(dst), before)
    both.close()
    only.close()


# ---- the demo ---------------------------------------------------------------------------------------------------------------------
def test_soil_hydrology_demo(tmp_path):
    """examples/soil_hydrology_demo.cc builds and runs: a day of rain on six columns, the budget of the stores closed."""
    out = run_demo(build_demo("soil_hydrology_demo", tmp_path), timeout=120)
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 8 and "soil hydrology, 48 steps" in lines[0]
    soil0, soil1 = (np.array([float(ln.split()[i]) for ln in lines[2:]]) for i in (3, 4))
    assert (soil1 != soil0).all()  # the rain wetted the soil
