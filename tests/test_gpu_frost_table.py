"""The frost table and the perched water table on the device (include/elmk.h "soil hydrology", F'): k_soil_hydrology<true> against the host
restatement (elmkernels_amd/hydrology.py: step with frost=) bit for bit in both builds, on generated columns that take every branch; a
six-step chain through the physics; the stage inside elmk_run against the stepwise calls, graph on and off, across an enable and a clear;
exact restarts with the version-4 image; every refusal; the accounting of the rows; the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests.hydrology_cases import (BRANCHES, CHAIN_STEPS, FROST_BRANCHES, Count, _new, _new_frost, _physics, add_frost, clear_snow,
                                   generated_frost, prepare)
from tests.run_cases import DT, NREC, SERIES, _inputs, device, same, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo

pytestmark = pytest.mark.gpu

STEP_FIELDS = hy.READS + ("h2osoi_vol", "t_soisno")


def _host_step(D, hit=None, lib_path=None, frost=True):
    """hydrology.step on what the device holds -> the fields, the rows and the extension's rows it must hold afterwards."""
    return hy.step({k: D[k] for k in STEP_FIELDS}, D.soil_hydrology_rows(), DT, hit, stored=np.float32 if lib_path else None,
                   frost=D.soil_hydrology_frost_rows() if frost else None)


def _assert_step(D, others, flags, want, want_rows, want_frost, what=""):
    got_rows, got_frost = D.soil_hydrology_rows(), D.soil_hydrology_frost_rows()
    for w in range(hy.NROWS):
        assert bits(got_rows[w]) == bits(want_rows[w]), (what, "row", w)
    for w in range(hy.FROST_NROWS):
        assert bits(got_frost[w]) == bits(want_frost[w]), (what, "frost row", w)
    for k in hy.WRITES:
        assert same(D[k], want[k]), (what, k)
    for k, v in others.items():
        assert same(D[k], v), (what, k)
    assert D.error_summary() == flags, what  # (no error bit is raised)


@pytest.mark.parametrize("n", [1001, 4700])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_one_step_equals_the_restatement(n, lib_path):
    """1001: partial waves and a partial workgroup; 4700: several workgroups, and thaw fronts that cycle through the layers in
    consecutive columns, so that every wave runs branches A and B under predicates.  Every written field, all 23 + 4 rows and err_flags
    against hydrology.step, every other field untouched; the restatement says that every branch was taken."""
    cols, scal, soil, rows, frost = generated_frost(n, 300 + n, full=True)
    D = _new_frost(cols, scal, soil, rows, frost, lib_path)
    assert D.level_stride != n
    assert bits(D.soil_hydrology_frost_rows()) == bits(np.where(np.arange(hy.FROST_NROWS)[:, None] == hy.Q_PERCH_MAX, frost, 0.0))
    hit = Count()
    want, want_rows, want_frost = _host_step(D, hit, lib_path)
    assert all(hit.get(k, 0) >= 20 for k in FROST_BRANCHES), {k: hit.get(k, 0) for k in FROST_BRANCHES}
    assert BRANCHES - {"drain_aquifer", "drain_soil"} <= set(hit)
    others = {k: D[k] for k in D.fields if k not in hy.WRITES}
    flags = D.error_summary()
    D.soil_hydrology(DT)
    _assert_step(D, others, flags, want, want_rows, want_frost)
    part = D.soil_hydrology_frost_read(hy.ZWT_PERCHED, col0=n // 2, n=n - n // 2)
    assert bits(part) == bits(want_frost[hy.ZWT_PERCHED][n // 2:])
    D.close()


@pytest.fixture(scope="module")
def chain_inputs():
    return generated_frost(1001, 77, full=True, chain=True)


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_six_step_chain_equals_the_restatement(chain_inputs, lib_path):
    """elmk_advance_physics, then the stage, six times: after every stage the device against hydrology.step on what the device held
    before it (the soil temperature is the physics' from the second step on)."""
    cols, scal, soil, rows, frost = chain_inputs
    D = _new_frost(cols, scal, soil, rows, frost, lib_path)
    hit = set()
    for s in range(CHAIN_STEPS):
        _physics(D)
        want, want_rows, want_frost = _host_step(D, hit, lib_path)
        others = {k: D[k] for k in D.fields if k not in hy.WRITES}
        flags = D.error_summary()
        D.soil_hydrology(DT)
        _assert_step(D, others, flags, want, want_rows, want_frost, s)
    assert {"frost_A", "frost_B_perched", "frost_B_none", "perched_ends_in_layer"} <= hit
    D.close()


# ---- the run ----------------------------------------------------------------------------------------------------------------------
NCOL = 200
NSTEPS = 4


@pytest.fixture(scope="module")
def base():
    b = _inputs(NCOL, 431)
    clear_snow(b[0])
    rows = prepare(b[0], 432)
    frost = add_frost(b[0], rows, 433)
    return b, rows, frost


def _context(base, graph, lib_path=None, frost=True, hydrology=True):
    b, rows, fr = base
    if not hydrology:
        D = device(b, lib_path=lib_path)
    elif frost:
        D = _new_frost(b[0], b[1], b[2], rows, fr, lib_path, b[3], b[4])
    else:
        D = _new(b[0], b[1], b[2], rows, lib_path, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    return D


def _snapshot(D, rows=True, frost=True):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    if rows:
        out["rows"] = D.soil_hydrology_rows()
    if frost:
        out["frost"] = D.soil_hydrology_frost_rows()
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
    """elmk_run with ELMK_RUN_HYDROLOGY on a context with the extension against the stepwise calls: the diagnostics rows, every state
    field, every row of the feature and of the extension.  Graph on and off therefore give the same bits."""
    want_diag, want = stepwise_result
    B = _context(base, graph)
    B.run(DT, schedule(NSTEPS), st.RUN_HYDROLOGY)
    for g, w in zip(B.run_diagnostics(), want_diag):
        assert same(g, w)
    got = _snapshot(B)
    _assert_same(got, want)
    assert np.isfinite(got["frost"]).all() and (got["frost"][hy.QFLX_DRAIN_PERCHED] != 0.0).sum() >= 20
    B.close()


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
def test_the_captured_run_step_follows_the_extension(base, graph):
    """One-step runs with the extension, after a clear, and after a second enable, on one context whose step is replayed from a
    captured graph: each against the stepwise calls on a context that takes the same turns.  The cleared step is the plain stage."""
    b, rows, frost = base
    S = schedule(3)
    A = _context(base, False)
    B = _context(base, graph)
    changed = []
    for s, turn in enumerate(("enabled", "cleared", "enabled again")):
        for D in (A, B):
            if turn == "cleared":
                D.soil_hydrology_frost_clear()
            elif turn == "enabled again":
                D.soil_hydrology_frost_enable(2.0 * frost[hy.Q_PERCH_MAX])
        liq0 = A["h2osoi_liq"]
        diag = stepwise(A, b[5], S[s:s + 1], st.RUN_HYDROLOGY)
        B.run(DT, S[s:s + 1], st.RUN_HYDROLOGY)
        for g, w in zip(B.run_diagnostics(), diag):
            assert same(g, w), turn
        _assert_same(_snapshot(B, frost=turn != "cleared"), _snapshot(A, frost=turn != "cleared"))
        changed.append(not same(A["h2osoi_liq"], liq0))
        if turn == "cleared":
            with pytest.raises(L.ElmkError):
                B.soil_hydrology_frost_read(hy.FROST_TABLE)
    assert all(changed)
    got = B.soil_hydrology_frost_rows()
    assert bits(got[hy.Q_PERCH_MAX]) == bits(2.0 * frost[hy.Q_PERCH_MAX]) and (got[hy.QFLX_DRAIN_PERCHED] != 0.0).any()
    A.close()
    B.close()


def test_restart_n_plus_n_equals_2n(base):
    """Two steps, an image, a fresh context with the extension, two more steps: the bits of four steps in one context.  The image is
    the version-4 image: byte for byte the size of the image of a context with the hydrology alone."""
    b, rows, frost = base
    S4 = schedule(NSTEPS)
    A = _context(base, True)
    A.run(DT, S4, st.RUN_HYDROLOGY)
    want = _snapshot(A)
    A.close()
    P = _context(base, True, frost=False)
    B = _context(base, True)
    assert B.restart_size() == P.restart_size()
    P.close()
    B.run(DT, S4[:2], st.RUN_HYDROLOGY)
    img = B.restart_save()
    assert img.size == B.restart_size()
    p = R.verify(img)
    assert int(p["header"]["version"]) == R.VERSION_HYDROLOGY == 4
    assert [(int(s["kind"]), int(s["id"])) for s in p["sections"][-2:]] == [(R.HYDROLOGY_SECTION, hy.ZWT), (R.HYDROLOGY_SECTION, hy.WA)]
    B.soil_hydrology_frost_clear()
    assert B.restart_size() == img.size
    B.close()
    C_ = _new_frost(b[0], b[1], b[2], np.where(np.arange(hy.NROWS)[:, None] < 2, 1.0, rows), frost, None, b[3], b[4])
    C_.set_graph(True)
    C_.run_reserve(NREC, 2 * NSTEPS)
    upload_series(C_, b[5])
    C_.restart_load(img)
    C_.run(DT, S4[2:], st.RUN_HYDROLOGY)
    _assert_same(_snapshot(C_), want)
    C_.close()


def test_refusals_change_nothing(base):
    b, rows, frost = base
    q = frost[hy.Q_PERCH_MAX]
    D = _context(base, True, hydrology=False)

    def state(with_rows):
        return _snapshot(D, rows=with_rows, frost=False), D.device_bytes, D.restart_size()

    def unchanged(a, b_):
        _assert_same(a[0], b_[0])
        assert a[1:] == b_[1:]

    before = state(False)
    for call in (lambda: D.soil_hydrology_frost_enable(q), lambda: D.soil_hydrology_frost_read(hy.FROST_TABLE)):  # without the hydrology
        with pytest.raises(L.ElmkError):
            call()
    D.soil_hydrology_frost_clear()  # nothing to free: OK
    unchanged(before, state(False))
    D.soil_hydrology_enable()
    D.soil_hydrology_set_params(rows[hy.HKSAT:hy.HKSAT + hy.N], rows[hy.WTFACT], rows[hy.H2OSFC_THRESH], rows[hy.K_WET], rows[hy.RSUB_TOP_MAX])
    D.soil_hydrology_init(rows[hy.ZWT], rows[hy.WA])
    before = state(True)
    for call in (lambda: D.soil_hydrology_frost_enable(None), lambda: D.soil_hydrology_frost_read(hy.FROST_TABLE)):  # null; not enabled
        with pytest.raises(L.ElmkError):
            call()
    unchanged(before, state(True))
    # a stream being captured: enable is refused
    buf = np.zeros(NCOL)
    with captured(D):
        rcs = [D.lib.elmk_soil_hydrology_frost_enable(D.ctx, q.ctypes.data_as(C.c_void_p))]
    assert rcs == [-1]  # ELMK_E_INVALID
    unchanged(before, state(True))
    D.soil_hydrology_frost_enable(q)
    assert D.device_bytes - before[1] == hy.FROST_NROWS * 8 * D.level_stride and D.restart_size() == before[2]
    f0 = D.soil_hydrology_frost_rows()
    before = state(True)
    with pytest.raises(L.ElmkError):  # twice
        D.soil_hydrology_frost_enable(q)
    for call in (lambda: D.soil_hydrology_frost_read(hy.FROST_NROWS), lambda: D.soil_hydrology_frost_read(-1),
                 lambda: D.soil_hydrology_frost_read(hy.FROST_TABLE, col0=NCOL, n=1), lambda: D.soil_hydrology_frost_read(hy.FROST_TABLE, col0=NCOL - 1, n=2)):
        with pytest.raises(L.ElmkError):
            call()
    # a stream being captured: read, clear, enable and the hydrology's clear are refused
    with captured(D):
        rcs = [D.lib.elmk_soil_hydrology_frost_read(D.ctx, hy.FROST_TABLE, buf.ctypes.data_as(C.c_void_p), 0, NCOL),
               D.lib.elmk_soil_hydrology_frost_clear(D.ctx), D.lib.elmk_soil_hydrology_frost_enable(D.ctx, q.ctypes.data_as(C.c_void_p)),
               D.lib.elmk_soil_hydrology_clear(D.ctx)]
    assert rcs == [-1] * 4, rcs
    unchanged(before, state(True))
    assert bits(D.soil_hydrology_frost_rows()) == bits(f0)
    D.close()


def test_accounting_and_a_cleared_context(base):
    """Enable adds exactly 4 x 8 x level_stride bytes and clear returns them; elmk_soil_hydrology_clear returns both sets; and a context
    that enabled and cleared the extension gives, in the next step, the bits of hydrology.step without `frost`."""
    b, rows, frost = base
    plain = device(b)
    bytes0 = plain.device_bytes
    plain.close()
    D = _new(b[0], b[1], b[2], rows, None, b[3], b[4])
    bytes1, size1 = D.device_bytes, D.restart_size()
    assert bytes1 - bytes0 == hy.NROWS * 8 * D.level_stride
    D.soil_hydrology_frost_enable(frost[hy.Q_PERCH_MAX])
    assert D.device_bytes - bytes1 == 4 * 8 * D.level_stride and D.restart_size() == size1
    _physics(D)
    D.soil_hydrology(DT)
    assert (D.soil_hydrology_frost_read(hy.QFLX_DRAIN_PERCHED) != 0.0).any()
    D.soil_hydrology_frost_clear()
    assert D.device_bytes == bytes1 and D.restart_size() == size1
    _physics(D)
    want, want_rows = hy.step({k: D[k] for k in STEP_FIELDS}, D.soil_hydrology_rows(), DT)
    others = {k: D[k] for k in D.fields if k not in hy.WRITES}
    D.soil_hydrology(DT)
    assert bits(D.soil_hydrology_rows()) == bits(want_rows)
    for k in hy.WRITES:
        assert same(D[k], want[k]), k
    for k, v in others.items():
        assert same(D[k], v), k
    D.soil_hydrology_frost_enable(frost[hy.Q_PERCH_MAX])
    assert D.device_bytes - bytes1 == 4 * 8 * D.level_stride
    D.soil_hydrology_clear()  # both sets
    assert D.device_bytes == bytes0
    with pytest.raises(L.ElmkError):
        D.soil_hydrology_frost_read(hy.FROST_TABLE)
    D.soil_hydrology_enable()  # and the extension does not come back with the hydrology
    assert D.device_bytes == bytes1
    with pytest.raises(L.ElmkError):
        D.soil_hydrology_frost_read(hy.FROST_TABLE)
    D.close()


# ---- the demo ---------------------------------------------------------------------------------------------------------------------
def test_permafrost_hydrology_demo(tmp_path):
    """examples/permafrost_hydrology_demo.cc builds and runs: four steps on five columns, finite values, the thaw depth and the perched
    table at or above the frost table, perched drainage in some column of every step."""
    out = run_demo(build_demo("permafrost_hydrology_demo", tmp_path), timeout=120)
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2 + 4 * 5 and "permafrost hydrology, 4 steps" in lines[0]
    v = np.array([[float(x) for x in ln.split()] for ln in lines[2:]])
    assert np.isfinite(v).all() and (v[:, 2] <= v[:, 3]).all() and (v[:, 4] <= v[:, 3]).all() and (v[:, 5] >= 0.0).all()
    for s in range(4):
        assert (v[v[:, 0] == s][:, 5] > 0.0).any()
    assert (v[v[:, 0] == 3][:, 3] > v[v[:, 0] == 0][:, 3]).all()  # the thaw front moved down
