"""Active layer thickness on the device (include/elmk.h "active layer thickness"): k_active_layer against the numpy restatement
(elmkernels_amd/active_layer.py) bit for bit in both builds, chained updates through the annual rollover of both hemispheres, the
update inside elmk_run against the stepwise calls, exact restarts (also across a change of decomposition), every refusal, no effect on
anything else, and the demo."""
import ctypes as C
import struct

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import accum
from elmkernels_amd import active_layer as al
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests import helpers as H
from tests.active_layer_cases import TFRZ, columns
from tests.run_cases import DT, NREC, SERIES, _inputs, demo_records, device, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo, same, state_blob

pytestmark = pytest.mark.gpu

ROWS = (al.ALT, al.ALTMAX, al.ALTMAX_LASTYEAR)
INDX = ("altmax_indx", "altmax_lastyear_indx")


def _lat(n, seed):
    """Both hemispheres, and some columns at lat == 0 (+0.0 and -0.0), which go south."""
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-1.4, 1.4, n)
    lat[::7] = 0.0
    lat[3::14] = -0.0
    return lat, rng.uniform(0.0, 6.0, n)


def _soil(n, seed):
    """columns() of the host test: the hand-built columns first, the rest random around tfrz; then, inside every wave, columns that
    leave the search at the first level (the bottom layer thawed) beside columns that walk all fifteen (everything frozen)."""
    t, z = columns(n, seed)
    c = np.arange(n)
    tail = c >= 64 if n > 64 else np.zeros(n, bool)
    t[19, tail & (c % 3 == 0)] = 280.0
    t[5:, tail & (c % 3 == 1)] = 268.0 - 0.125 * np.arange(15)[:, None]
    return t, z


def _rows(D):
    return [D.active_layer_read(w) for w in ROWS] + [D[k] for k in INDX]


def _seen(D):
    """t_soisno and zsoi as the device holds them ([20, n] float64: rounded to fp32 in the fp32-state build)."""
    return [np.ascontiguousarray(D[k].T).astype(np.float64) for k in ("t_soisno", "zsoi")]


@pytest.mark.parametrize("n", [1, 193, 600])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_update_equals_the_restatement(n, lib_path):
    """One lane, a partial workgroup, three workgroups with a partial last wave.  Three updates from fresh soil columns (no rollover,
    NORTH, NORTH | SOUTH); after every one the three rows and both index fields against active_layer.update."""
    D = st.ELMState(n, lib_path=lib_path)
    assert D.level_stride == 64 * ((n + 63) // 64) and D.level_stride != n
    lat, lon = _lat(n, 3 + n)
    if n == 1:
        lat[0] = 0.5
    D.set_column_geography(lat, lon)
    north = al.north(lat)
    before = D.device_bytes
    D.active_layer_enable()
    assert D.device_bytes - before == 3 * 8 * D.level_stride
    D["altmax_indx"] = np.full(n, 5, np.int32)  # the reference driver's placeholders
    D["altmax_lastyear_indx"] = np.zeros(n, np.int32)
    rng = np.random.default_rng(n)
    am0, aly0 = 0.3 * rng.random(n), rng.random(n)
    D.active_layer_init(am0, aly0)
    want = [np.zeros(n), am0, aly0, np.full(n, 5, np.int32), np.zeros(n, np.int32)]
    for g, w in zip(_rows(D), want):
        assert bits(g) == bits(w)
    untouched = {k: D[k] for k in D.fields if k not in INDX + ("t_soisno", "zsoi")}
    ks = set()
    for step, roll in enumerate((0, al.ROLL_NORTH, al.ROLL_NORTH | al.ROLL_SOUTH)):
        t, z = _soil(n, 100 * n + step)
        if n == 1:  # one column: a thawed layer over a frozen one, the bottom layer thawed, everything frozen
            t[5:, 0] = [(275.15,) * 4 + (271.15,) * 11, (275.15,) * 15, (260.0,) * 15][step]
        D["t_soisno"] = t.T
        D["zsoi"] = z.T
        ts, zs = _seen(D)
        D.active_layer_update(roll)
        want = al.update(ts, zs, *want, north, roll)
        for i, (g, w) in enumerate(zip(_rows(D), want)):
            assert g.dtype == w.dtype and bits(g) == bits(w), (step, i)
        assert bits(_seen(D)[0]) == bits(ts) and bits(_seen(D)[1]) == bits(zs)  # the inputs are only read
        ks |= set(want[3].tolist())
    for k, v in untouched.items():
        assert same(D[k], v), k
    if n > 1:  # the columns did what they were built for
        t, z = _soil(n, 100 * n)
        if lib_path:
            t, z = t.astype(np.float32), z.astype(np.float32)
        zero, none = np.zeros(n), np.full(n, -1, np.int32)
        alt, _, _, ix, _ = al.update(t, z, zero, zero, zero, none, none, north, al.ROLL_NORTH | al.ROLL_SOUTH)
        assert ix[:16].tolist() == list(range(-1, 15)) and ix[17] == 7 and ix[18] == 2 and np.isnan(alt).any() and np.isinf(alt).any()
        assert ks >= set(range(-1, 15))
        wave = slice(64, 128)
        assert (ix[wave] == 14).any() and (ix[wave] == -1).any() and ((ix[wave] >= 0) & (ix[wave] < 14)).any()
    part = D.active_layer_read(al.ALTMAX, col0=n // 2, n=n - n // 2)
    assert bits(part) == bits(want[1][n // 2:])
    D.active_layer_clear()
    assert D.device_bytes == before
    assert bits(D["altmax_indx"]) == bits(want[3])  # the state fields keep their values
    D.close()


def test_six_chained_updates():
    """New t_soisno between the updates; rollovers 0, 0, NORTH, 0, SOUTH, NORTH | SOUTH over both hemispheres and lat == 0."""
    n = 193
    D = st.ELMState(n)
    lat, lon = _lat(n, 11)
    D.set_column_geography(lat, lon)
    north = al.north(lat)
    assert north.any() and (~north).any() and not north[lat == 0.0].any() and (lat == 0.0).sum() > 10
    D.active_layer_enable()
    al.cold_start(D)
    rng = np.random.default_rng(12)
    z = np.cumsum(0.05 + rng.random((20, n)), axis=0) - 1.0
    D["zsoi"] = z.T
    want = [np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, -1, np.int32), np.full(n, -1, np.int32)]
    for step, roll in enumerate((0, 0, al.ROLL_NORTH, 0, al.ROLL_SOUTH, al.ROLL_NORTH | al.ROLL_SOUTH)):
        t = TFRZ + 2.0 * rng.standard_normal((20, n)) - 0.35 * np.arange(20)[:, None] + 3.0
        if step == 2:
            t[:, ::5] = 250.0  # frozen through the northern rollover: the index resets to -1 and stays there
        D["t_soisno"] = t.T
        ts, zs = _seen(D)
        prev = [w.copy() for w in want]
        D.active_layer_update(roll)
        want = al.update(ts, zs, *want, north, roll)
        got = _rows(D)
        for i, (g, w) in enumerate(zip(got, want)):
            assert bits(g) == bits(w), (step, i)
        alt, am, aly, ix, ily = got
        rolled = ((roll & 1) != 0) & north | ((roll & 2) != 0) & ~north
        # inside a year the maximum only grows, and last year's rows stay
        assert (am[~rolled] >= prev[1][~rolled]).all() and bits(aly[~rolled]) == bits(prev[2][~rolled]) and bits(ily[~rolled]) == bits(prev[4][~rolled])
        # the right hemisphere only takes the old values, and starts again from this step's depth
        assert bits(aly[rolled]) == bits(prev[1][rolled]) and bits(ily[rolled]) == bits(prev[3][rolled])
        assert bits(am[rolled]) == bits(np.where(alt[rolled] > 0.0, alt[rolled], 0.0))
        assert (ix[rolled][alt[rolled] == 0.0] == -1).all()
        if roll:
            assert rolled.any() and (roll == 3 or (~rolled).any())
        if step == 2:
            frozen = rolled & (np.arange(n) % 5 == 0)
            assert frozen.any() and (ix[frozen] == -1).all() and (am[frozen] == 0.0).all() and (prev[3][frozen] >= 0).any()
    D.close()


def test_update_in_a_captured_graph():
    """elmk_active_layer_update captured on a caller's stream and replayed: stream-ordered, no host memory."""
    n = 193
    D = st.ELMState(n)
    lat, lon = _lat(n, 21)
    D.set_column_geography(lat, lon)
    D.active_layer_enable()
    al.cold_start(D)
    t, z = _soil(n, 22)
    D["t_soisno"], D["zsoi"] = t.T, z.T
    with captured(D) as cap:
        D.active_layer_update(al.ROLL_SOUTH)
        cap.end()
        assert not D.active_layer_read(al.ALT).any()  # captured, not run
        cap.replay(2)
        want = [np.zeros(n), np.zeros(n), np.zeros(n), np.full(n, -1, np.int32), np.full(n, -1, np.int32)]
        for _ in range(2):
            want = al.update(t, z, *want, al.north(lat), al.ROLL_SOUTH)
        for g, w in zip(_rows(D), want):
            assert bits(g) == bits(w)
    D.close()


# ---- the run -------------------------------------------------------------------------------------------------------------------------
NCOL = 200
NSTEPS = 4


def new_year_schedule(nsteps=NSTEPS):
    """Half-hour steps from 23:00 of 31 December: doy 364, 364, 0, 0; the third step starts at 00:00 of 1 January."""
    S = schedule(nsteps)
    for s in range(nsteps):
        ddoy = (364.0 + 46.0 / 48.0 + s / 48.0) % 365.0
        S[s]["decday"], S[s]["doy"] = ddoy + 1.0, int(ddoy)
    assert [int(x) for x in S["doy"][:4]] == [364, 364, 0, 0][:nsteps]
    assert [al.rollover(int(p["doy"]), float(p["decday"])) for p in S][:4] == [0, 0, al.ROLL_NORTH, 0][:nsteps]
    return S


@pytest.fixture(scope="module")
def base():
    b = _inputs(NCOL, 231)
    cols = b[0]
    # a thaw front in most columns: warm at the top, colder with depth, some frozen columns and some thawed to the bottom
    rng = np.random.default_rng(5)
    t = TFRZ + 6.0 * rng.random((NCOL, 1)) - 0.6 * np.arange(20)[None, :] + 2.0
    t[::9] = 262.0
    t[4::9] = 281.0
    cols["t_soisno"] = t
    cols["altmax_indx"] = np.full(NCOL, 5, np.int32)
    cols["altmax_lastyear_indx"] = np.zeros(NCOL, np.int32)
    assert (np.sin(b[3]) > 0.0).any() and (np.sin(b[3]) <= 0.0).any()
    return b


def _altmax0(n):
    return 0.01 * np.arange(n), 5.0 - 0.02 * np.arange(n)


def _context(base, graph, entries=False):
    D = device(base)
    D.set_graph(graph)
    D.active_layer_enable()
    D.active_layer_init(*_altmax0(D.ncols))
    out = None
    if entries:
        out = (D.accum_add("altmax_indx", accum.RUNMEAN, 3), D.history_add(0, "altmax_indx", "max"), D.history_add(0, "altmax_lastyear_indx", "max"))
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, base[5])
    return D, out


def _snapshot(D, entries=None):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    for w in ROWS:
        out[f"row{w}"] = D.active_layer_read(w)
    if entries:
        out["accum"], out["count"] = D.accum_read(entries[0])
        out["hist1"], out["hist2"], out["samples"] = D.history_read(entries[1]), D.history_read(entries[2]), D.history_count(0)
    return out


def _assert_same(a, b, c0=None, m=None):
    assert a.keys() == b.keys()
    for k, v in a.items():
        w = b[k]
        if c0 is not None and isinstance(w, np.ndarray):
            w = w[c0:c0 + m]
        assert same(v, w) if isinstance(v, np.ndarray) else v == w, k


@pytest.fixture(scope="module")
def stepwise_result(base):
    out = {}
    for entries in (False, True):
        A, e = _context(base, False, entries)
        diag = stepwise(A, base[5], new_year_schedule(), st.RUN_ALT | ((st.RUN_ACCUM | st.RUN_HISTORY) if entries else 0))
        out[entries] = (diag, _snapshot(A, e))
        A.close()
    return out


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "nograph"])
@pytest.mark.parametrize("entries", [False, True], ids=["alt", "alt+accum+history"])
def test_run_equals_stepwise(base, stepwise_result, graph, entries):
    """elmk_run with ELMK_RUN_ALT over four steps that cross 00:00 of 1 January against the stepwise calls with
    elmk_active_layer_update(rollover(...)) after each step: every state field and the three rows.  With ELMK_RUN_ACCUM |
    ELMK_RUN_HISTORY an accumulator and a MAX tape of altmax_indx see the step's new index."""
    want_diag, want = stepwise_result[entries]
    B, e = _context(base, graph, entries)
    B.run(DT, new_year_schedule(), st.RUN_ALT | ((st.RUN_ACCUM | st.RUN_HISTORY) if entries else 0))
    for g, w in zip(B.run_diagnostics(), want_diag):
        assert same(g, w)
    got = _snapshot(B, e)
    _assert_same(got, want)
    B.close()
    # what the run did: the northern columns rolled over in step 2, the southern ones kept their year
    north = al.north(base[3])
    am0, aly0 = _altmax0(NCOL)
    assert bits(got["row2"][~north]) == bits(aly0[~north]) and (got["altmax_lastyear_indx"][~north] == 0).all()
    assert (got["row1"][~north] >= am0[~north]).all()
    assert (got["altmax_lastyear_indx"][north] != 0).any() and (got["row2"][north] != aly0[north]).all()
    assert (got["altmax_indx"] == -1).any() and (got["altmax_indx"] == 14).any() and ((got["altmax_indx"] > 0) & (got["altmax_indx"] < 14)).any()
    if entries:
        assert got["count"] == NSTEPS and got["samples"] == NSTEPS
        # the tape saw the new values: the last-year index of a northern column is the maximum it took in step 2, never the 0 before
        assert bits(got["hist2"][north]) == bits(np.maximum(got["altmax_lastyear_indx"][north], 0).astype(np.float64))
        assert (got["hist1"] >= got["altmax_indx"]).all() and (got["hist1"][north] >= got["altmax_lastyear_indx"][north]).all()


def test_no_effect_elsewhere(base):
    """One step after an update of the feature leaves every field but the two indices as a context without the feature has it."""
    steps = new_year_schedule()[:1]
    A = device(base)
    B = device(base)
    before = B.device_bytes
    B.active_layer_enable()
    assert B.device_bytes - before == 3 * 8 * B.level_stride and A.device_bytes == before
    B.active_layer_update(al.ROLL_NORTH | al.ROLL_SOUTH)
    assert not same(A["altmax_indx"], B["altmax_indx"]) and not same(A["altmax_lastyear_indx"], B["altmax_lastyear_indx"])
    wa, wb = stepwise(A, base[5], steps), stepwise(B, base[5], steps)
    B.active_layer_update(0)
    for g, w in zip(wa, wb):
        assert same(g, w)
    for k in A.fields:
        if k not in INDX:
            assert same(A[k], B[k]), k
    A.close()
    B.close()


# ---- restart -------------------------------------------------------------------------------------------------------------------------
N = NSTEPS // 2
FLAGS = st.RUN_ALT | st.RUN_ACCUM | st.RUN_HISTORY


def _sub(base, c0, n):
    cols, scal, soil, lat, lon, rec = base
    return ({k: v[c0:c0 + n] for k, v in cols.items()}, scal, soil, lat[c0:c0 + n], lon[c0:c0 + n],
            {k: v[:, c0:c0 + n] for k, v in rec.items()})


def _blank(D):
    for name, (fid, nlev, dt) in D.fields.items():
        D.fill(name, np.nan if dt == np.float64 else 3.0)
    D.active_layer_init(np.full(D.ncols, np.nan), np.full(D.ncols, np.nan))


@pytest.fixture(scope="module")
def continuous(base):
    """2N steps that never stop (the rollover is step N), and the image after the first N."""
    A, e = _context(base, True, True)
    A.run(DT, new_year_schedule()[:N], FLAGS)
    img = A.restart_save()
    assert img.size == A.restart_size()
    A.run(DT, new_year_schedule()[N:], FLAGS)
    snap = _snapshot(A, e)
    A.close()
    return img, snap


def test_exact_restart(base, continuous):
    img, want = continuous
    p = R.verify(img)
    assert int(p["header"]["version"]) == 3 and [int(x) for x in p["accum"]["nsteps"]] == [N]
    kinds = [int(s["kind"]) for s in p["sections"]]
    assert kinds[-3:] == [R.ALT_SECTION] * 3 and kinds[-4] == R.ACCUM_SECTION and [int(s["id"]) for s in p["sections"][-3:]] == [0, 1, 2]
    D, e = _context(base, True, True)
    _blank(D)
    D.restart_load(img)
    D.run(DT, new_year_schedule()[N:], FLAGS)
    _assert_same(_snapshot(D, e), want)
    D.close()


def test_restart_across_a_change_of_decomposition(base, continuous):
    img, want = continuous
    parts = []
    for c0, m in ((0, 120), (120, 80)):
        D, e = _context(_sub(base, c0, m), True, True)
        _blank(D)
        D.restart_load(R.slice(img, c0, m), c0)
        D.run(DT, new_year_schedule()[N:], FLAGS)
        _assert_same(_snapshot(D, e), want, c0, m)
        parts.append(D.restart_save(c0))
        D.close()
    full = R.verify(R.merge(parts[::-1]))
    assert int(full["header"]["version"]) == 3 and int(full["header"]["ncols"]) == NCOL
    for s, d in zip(full["sections"], full["data"]):
        if int(s["kind"]) == R.ALT_SECTION:
            assert bits(d.reshape(-1)) == bits(want[f"row{int(s['id'])}"])


def test_versions_do_not_mix(base):
    """enable then clear saves the bytes a never-enabled context saves; a version-3 image into a plain context and a version-1 image into
    an enabled one are refused with state and rows unchanged."""
    D = device(base)
    size0, bytes0 = D.restart_size(), D.device_bytes
    img1 = D.restart_save()
    assert int(R.verify(img1)["header"]["version"]) == 1 and img1.size == size0
    D.active_layer_enable()
    assert D.restart_size() > size0 and D.device_bytes > bytes0
    D.active_layer_clear()
    assert D.restart_size() == size0 and D.device_bytes == bytes0
    assert bits(D.restart_save()) == bits(img1)
    # an enabled context without accumulator entries: version 3 with the count word 0
    E = device(base)
    E.active_layer_enable()
    E.active_layer_init(*_altmax0(NCOL))
    E.active_layer_update(al.ROLL_SOUTH)
    img3 = E.restart_save()
    p = R.verify(img3)
    assert int(p["header"]["version"]) == 3 and p["accum"].size == 0
    assert struct.unpack("<II", img3[R.HEADER.itemsize:R.HEADER.itemsize + 8].tobytes()) == (0, 0)
    for s, d in zip(p["sections"][-3:], p["data"][-3:]):
        assert bits(d.reshape(-1)) == bits(E.active_layer_read(int(s["id"])))
    # refused both ways, nothing written
    D["t_grnd"] = np.full(NCOL, 250.0)
    state = {k: D[k] for k in D.fields}
    assert D.lib.elmk_restart_load(D.ctx, 0, img3.ctypes.data, img3.size) == -1
    assert b"version-3" in D.lib.elmk_last_error(D.ctx)
    for k, v in state.items():
        assert same(D[k], v), k
    E["t_grnd"] = np.full(NCOL, 251.0)
    state = {k: E[k] for k in E.fields}
    rows = [E.active_layer_read(w) for w in ROWS]
    assert E.lib.elmk_restart_load(E.ctx, 0, img1.ctypes.data, img1.size) == -1
    for k, v in state.items():
        assert same(E[k], v), k
    for w in ROWS:
        assert bits(E.active_layer_read(w)) == bits(rows[w])
    # and the image loads where it belongs
    E.active_layer_init(None, None)
    E.restart_load(img3)
    for w in ROWS:
        assert bits(E.active_layer_read(w)) == bits(rows[w])
    assert same(E["t_grnd"], state["t_grnd"]) is False
    D.close()
    E.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(base):
    lib = L.load()
    # without the feature, and without a geography
    P = st.ELMState(NCOL)
    buf = np.zeros(NCOL)
    ptr = buf.ctypes.data_as(C.c_void_p)
    indx = P["altmax_indx"]
    assert lib.elmk_active_layer_update(P.ctx, 0) == -1 and b"not enabled" in lib.elmk_last_error(P.ctx)
    assert lib.elmk_active_layer_read(P.ctx, 0, ptr, 0, NCOL) == -1
    assert lib.elmk_active_layer_init(P.ctx, None, None) == -1
    assert lib.elmk_active_layer_clear(P.ctx) == 0  # nothing to free
    P.active_layer_enable()
    assert lib.elmk_active_layer_update(P.ctx, 0) == -1 and b"geography" in lib.elmk_last_error(P.ctx)
    assert same(P["altmax_indx"], indx) and not P.active_layer_read(al.ALTMAX).any()
    P.close()

    D = device(base)
    ctx = D.ctx
    D.run_reserve(NREC, NSTEPS)
    upload_series(D, base[5])
    a = np.ascontiguousarray(new_year_schedule(), dtype=st.RUN_STEP_DTYPE)
    indx = {k: D[k] for k in INDX}
    # the flag without enable: refused before anything is enqueued
    t_grnd = D["t_grnd"]
    assert lib.elmk_run(ctx, DT, a.ctypes.data_as(C.c_void_p), int(a.size), st.RUN_ALT) == -1
    assert b"ELMK_RUN_ALT" in lib.elmk_last_error(ctx) and same(D["t_grnd"], t_grnd)
    assert lib.elmk_run(ctx, DT, a.ctypes.data_as(C.c_void_p), int(a.size), 32) == -1  # the next bit is still unknown
    D.active_layer_enable()
    D.active_layer_init(*_altmax0(NCOL))
    D.active_layer_update(0)

    def state():
        return [D.active_layer_read(w) for w in ROWS] + [D[k] for k in INDX] + [np.array([D.device_bytes, D.restart_size()])]

    def unchanged(x, y):
        return all(bits(p) == bits(q) for p, q in zip(x, y))

    before = state()
    assert lib.elmk_active_layer_enable(ctx) == -1 and b"already enabled" in lib.elmk_last_error(ctx)  # enable twice
    assert unchanged(before, state())
    for roll in (4, 7, -1, 1 << 16):  # bad rollover bits
        assert lib.elmk_active_layer_update(ctx, roll) == -1, roll
    assert unchanged(before, state())
    for which in (-1, 3):  # bad row
        assert lib.elmk_active_layer_read(ctx, which, ptr, 0, NCOL) == -1, which
    for col0, m in ((1, NCOL), (-1, 10), (0, -1), (NCOL, 1)):  # bad column range
        assert lib.elmk_active_layer_read(ctx, al.ALT, ptr, col0, m) == -1, (col0, m)
    assert lib.elmk_active_layer_read(ctx, al.ALT, None, 0, 1) == -1 and lib.elmk_active_layer_read(ctx, al.ALT, None, 0, 0) == 0
    assert not buf.any() and unchanged(before, state())
    # a stream being captured: enable (on another context), init, read and clear are refused; nothing changes
    O = st.ELMState(NCOL)
    o_bytes = O.device_bytes
    with captured(D, O):
        rcs = [lib.elmk_active_layer_enable(O.ctx), lib.elmk_active_layer_init(ctx, None, None), lib.elmk_active_layer_read(ctx, 0, ptr, 0, NCOL),
               lib.elmk_active_layer_clear(ctx)]
    assert rcs == [-1] * 4, rcs
    assert unchanged(before, state()) and O.device_bytes == o_bytes
    assert lib.elmk_active_layer_read(O.ctx, 0, ptr, 0, NCOL) == -1  # O was never enabled
    O.close()
    # the context is still usable: the run with the flag equals the stepwise calls' rows
    D.run(DT, new_year_schedule()[:1], st.RUN_ALT)
    D.sync()
    assert (D.active_layer_read(al.ALTMAX) >= before[1]).all()
    D.close()


# ---- the demo ------------------------------------------------------------------------------------------------------------------------
def test_active_layer_demo(tmp_path):
    """examples/active_layer_demo.cc builds and runs 6 steps across 00:00 of 1 January: one run against the stepwise updates."""
    n = 320
    cols, scal, soil, lat, lon, rec = _inputs(n, 75, nrec=25)
    cols["t_soisno"] = TFRZ + 5.0 * np.random.default_rng(1).random((n, 1)) - 0.5 * np.arange(20)[None, :] + 2.0
    exe = build_demo("active_layer_demo", tmp_path)
    extra = demo_records(lat, lon, rec) + [("steps", new_year_schedule(6))]
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, extra))
    r = run_demo(exe, tmp_path / "state.bin")
    assert "bit-identical" in r.stdout and "ALTMAX_LASTYEAR" in r.stdout
