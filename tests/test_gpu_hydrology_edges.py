"""Soil hydrology on the device on the edge tier (tests/hydrology_cases.py: edge_columns): k_soil_hydrology<false> and <true> against
the host restatement (elmkernels_amd/hydrology.py: step) in both builds.  Every written field and every row bit for bit, where both
sides hold a NaN that counts as equal (the rows are canonical on both sides; a NaN of a state field keeps whatever sign and payload
the arithmetic gave it); every other field untouched.  The comparison is per column, and a third of the columns hold a NaN or an
infinity in one input: a poisoned column therefore cannot have moved its neighbours.

The sizes: one column, one wave less one, one wave (the level stride equals the column count: nothing is padded), one wave and one,
one workgroup, one workgroup and one, and a thousand; the step lengths 1 s, 1800 s and a day; the stage on what two steps of the
physics leave of the wide tier; and the tier inside elmk_run, graph on and off, against the stepwise calls."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import parity_cases as P
from tests.hydrology_cases import EDGE_CLASS_NAMES, _new, _new_frost, edge_columns, prepare
from tests.run_cases import DT, NREC, SERIES, _inputs, same, schedule, stepwise, upload_series

pytestmark = pytest.mark.gpu

LIBS = pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
FORMS = pytest.mark.parametrize("frost", [False, True], ids=["plain", "frost"])
SEED = 5


def same_or_nan(got, want):
    """Bit for bit, or NaN on both sides."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    eq = got.view(np.uint8).reshape(got.shape + (got.itemsize,)) == want.view(np.uint8).reshape(want.shape + (want.itemsize,))
    eq = eq.all(axis=-1)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    return bool(eq.all())


def _context(g, frost, lib_path, lat=None, lon=None):
    cols, scal, soil, rows = g[:4]
    return _new_frost(cols, scal, soil, rows, g[4], lib_path, lat, lon) if frost else _new(cols, scal, soil, rows, lib_path, lat, lon)


def _stage_against_the_host(D, frost, lib_path, dt, what=""):
    """One elmk_soil_hydrology against hydrology.step on what the device holds."""
    fields = {k: D[k] for k in hy.READS + ("h2osoi_vol",) + (("t_soisno",) if frost else ())}
    want = hy.step(fields, D.soil_hydrology_rows(), dt, stored=np.float32 if lib_path else None,
                   frost=D.soil_hydrology_frost_rows() if frost else None)
    others = {k: D[k] for k in D.fields if k not in hy.WRITES}
    flags = D.error_summary()
    D.soil_hydrology(dt)
    bad = []  # everything that differs, so that one run shows the whole of a disagreement
    got_rows = D.soil_hydrology_rows()
    for w in range(hy.NROWS):
        if not same_or_nan(got_rows[w], want[1][w]):
            bad.append(("row", w) + _first(got_rows[w], want[1][w]))
    if frost:
        got_frost = D.soil_hydrology_frost_rows()
        for w in range(hy.FROST_NROWS):
            if not same_or_nan(got_frost[w], want[2][w]):
                bad.append(("frost row", w) + _first(got_frost[w], want[2][w]))
    for k in hy.WRITES:
        if not same_or_nan(D[k], want[0][k]):
            bad.append((k,) + _first(D[k], want[0][k]))
    bad += [(k, "touched") for k, v in others.items() if not same(D[k], v)]
    assert not bad, (what, bad)
    assert D.error_summary() == flags, what
    return want


def _first(got, want):
    """The first column that differs, its edge class and the two values: what an assertion shows."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if not bad.any():
        bad = got.view(np.uint64) != want.view(np.uint64)
    i = int(np.argwhere(bad)[0][0]) if bad.any() else -1
    return i, EDGE_CLASS_NAMES[i % len(EDGE_CLASS_NAMES)], got[i].tolist(), want[i].tolist()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1001])
@FORMS
@LIBS
def test_the_edge_tier_equals_the_restatement(n, frost, lib_path):
    g = edge_columns(n, SEED, frost=frost, full=True)
    D = _context(g, frost, lib_path)
    assert (D.level_stride == n) == (n % 64 == 0)  # 64 and 256 run unpadded
    want = _stage_against_the_host(D, frost, lib_path, DT)
    if n >= len(EDGE_CLASS_NAMES):
        assert np.isnan(want[1][hy.ZWT]).any() and np.isfinite(want[1][hy.ZWT]).sum() > n // 2
    D.close()


@pytest.mark.parametrize("dt", [1.0, 86400.0])
@FORMS
@LIBS
def test_the_edge_tier_at_other_step_lengths(dt, frost, lib_path):
    """n = 257 holds every class of the tier once.  At 1 s the bound of h2osfc's runoff by what the store holds gives way to the
    rate; at a day the recharge and the drainage move whole layers."""
    g = edge_columns(257, SEED + 1, frost=frost, full=True)
    D = _context(g, frost, lib_path)
    _stage_against_the_host(D, frost, lib_path, dt)
    D.close()


@FORMS
@LIBS
def test_the_stage_on_what_the_physics_leaves_of_the_wide_tier(frost, lib_path):
    """Two steps of elmk_init_timestep and elmk_advance_physics on the wide state of parity_cases' W_advance (a thousand columns of
    it), then the stage: it runs on what the wide draw and its edge rows leave behind, and once more after a third step."""
    case = P.BY_NAME["W_advance"]
    n = 1000
    cols, scal, soil = P.state(P.Case(case.name, case.tier, n, case.seed, scalars=case.scalars), st.field_table())
    rows = prepare({k: np.array(v) for k, v in cols.items()}, case.seed + 1)  # the rows alone: the state stays the wide one
    lat, lon = synth.global_grid(n, seed=9)
    if frost:
        q = hy.q_perch_max(np.random.default_rng(case.seed + 2).uniform(0.5, 12.0, n))
        D = _new_frost(cols, scal, soil, rows, np.where(np.arange(hy.FROST_NROWS)[:, None] == hy.Q_PERCH_MAX, q, 0.0), lib_path, lat, lon)
    else:
        D = _new(cols, scal, soil, rows, lib_path, lat, lon)
    for s in range(2):
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
    _stage_against_the_host(D, frost, lib_path, DT, "after two steps")
    st.kokkos_init_timestep(D)
    st.advance_physics(D, DT)
    _stage_against_the_host(D, frost, lib_path, DT, "after the third")
    D.close()


# ---- the run ----------------------------------------------------------------------------------------------------------------------
NCOL = 200
NSTEPS = 2


def _run_context(frost, lib_path, graph):
    b = _inputs(NCOL, SEED + 2)  # (the generator's state of this seed: the tier below is built on the same draw)
    g = edge_columns(NCOL, SEED + 2, frost=frost, full=True)
    D = _context(g, frost, lib_path, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, b[5])
    return D, b[5]


def _snapshot(D, frost):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out["rows"] = D.soil_hydrology_rows()
    if frost:
        out["frost"] = D.soil_hydrology_frost_rows()
    return out


@FORMS
@LIBS
def test_run_equals_stepwise_on_the_edge_tier(frost, lib_path):
    """elmk_run with ELMK_RUN_HYDROLOGY over two steps on the edge tier, graph on and graph off, against the stepwise calls: the
    diagnostics rows, every state field and every row, bit for bit (the device against itself: NaN for NaN)."""
    A, rec = _run_context(frost, lib_path, False)
    want_diag = stepwise(A, rec, schedule(NSTEPS), st.RUN_HYDROLOGY)
    want = _snapshot(A, frost)
    A.close()
    for graph in (True, False):
        B, _ = _run_context(frost, lib_path, graph)
        B.run(DT, schedule(NSTEPS), st.RUN_HYDROLOGY)
        for g_, w in zip(B.run_diagnostics(), want_diag):
            assert same(g_, w), graph
        got = _snapshot(B, frost)
        assert got.keys() == want.keys()
        for k, v in want.items():
            assert same(got[k], v), (graph, k)
        B.close()
    assert np.isfinite(want["rows"][hy.ZWT]).sum() > NCOL // 2
