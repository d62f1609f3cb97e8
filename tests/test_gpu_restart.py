"""Exact restarts on the device (include/elmk.h "restart"): E3SM's ERS test - 2N steps against N steps, a save, a fresh context
whose every field outside the image is poisoned, a load and N more steps - bit for bit in every field, every history result,
the tape counts and the error summary; a change of column decomposition through restart.merge / restart.slice; the image's
contents against elmk_download; every refusal of elmk_restart_load, each leaving the context as it was; and the matrix of the
optional features: which image loads into which context."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests import helpers as H
from tests import restart_cases as RC
from tests.run_cases import DT, IMAGE_CLASSES, NREC, NSTEPS, _inputs, demo_records, device, poison, schedule, stepwise, upload_series
from tests.support import build_demo, captured, run_demo, same, state_blob

pytestmark = pytest.mark.gpu

N = NSTEPS // 2


@pytest.fixture(scope="module")
def base():
    return _inputs(3001, 97)


def _sub(base, c0, n):
    cols, scal, soil, lat, lon, rec = base
    return ({k: v[c0:c0 + n] for k, v in cols.items()}, scal, soil, lat[c0:c0 + n], lon[c0:c0 + n],
            {k: v[:, c0:c0 + n] for k, v in rec.items()})


def _output_map(n, per=7):
    cells = np.arange(n) // per
    ncells = int(cells[-1]) + 1
    ptr = np.searchsorted(cells, np.arange(ncells + 1)).astype(np.int64)
    w = 1.0 + 0.01 * (np.arange(n) % 5)
    return ptr, np.arange(n, dtype=np.int32), w


def _history(D, gridded=True):
    """Entries on two tapes with every op (and gridded ones); returns their ids."""
    ids = [D.history_add(0, "t_grnd", "avg"), D.history_add(0, "t_soisno", "max"), D.history_add(0, "h2osno", "min"),
           D.history_add(0, "eflx_sh_tot", "sum"), D.history_add(1, "snl", "inst"), D.history_add(1, "h2osoi_liq", "avg")]
    if gridded:
        D.set_output_grid(*_output_map(D.ncols))
        ids += [D.gridded_history_add(1, "t_grnd", "avg"), D.gridded_history_add(1, "eflx_lh_tot", "max")]
    return ids


def _snapshot(D, ids):
    out = {k: D[k] for k in D.fields}
    out["hist"] = [D.history_read(e) if D.history_count(0 if e < 4 else 1) > 0 else None for e in ids]
    out["counts"] = [D.history_count(t) for t in range(st.HIST_MAX_TAPES)]
    out["errors"] = D.error_summary()
    return out


def _assert_same(a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        if k == "hist":
            for x, y in zip(a[k], b[k]):
                assert (x is None and y is None) or same(x, y), "history"
        elif k in ("counts", "errors"):
            assert a[k] == b[k], k
        else:
            assert same(a[k], b[k]), k


def _fresh(base, gridded=True, graph=False, lib_path=None):
    D = device(base, lib_path=lib_path)
    D.set_graph(graph)
    ids = _history(D, gridded)
    poison(D)
    return D, ids


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_ers_stepwise(base, lib_path):
    """ERS through the stepwise calls, history with every op on two tapes and gridded entries."""
    rec = base[5]
    sch = schedule()
    A = device(base, lib_path=lib_path)
    ids = _history(A)
    stepwise(A, rec, sch, st.RUN_HISTORY)
    B = device(base, lib_path=lib_path)
    _history(B)
    stepwise(B, rec, sch[:N], st.RUN_HISTORY)
    img = B.restart_save()
    B.close()
    R.verify(img)
    Cx, ids_c = _fresh(base, lib_path=lib_path)
    Cx.restart_load(img)
    assert [Cx.history_count(t) for t in range(4)] == [N, N, 0, 0]
    stepwise(Cx, rec, sch[N:], st.RUN_HISTORY)
    # the series inputs hold the last step's records in both
    _assert_same(_snapshot(A, ids), _snapshot(Cx, ids_c))
    A.close()
    Cx.close()


def test_ers_run_with_graph(base):
    """ERS through elmk_run with graphs on: N steps in one run, save, a fresh poisoned context, load, the other N in one run."""
    rec = base[5]
    sch = schedule()
    A = device(base)
    A.set_graph(True)
    ids = _history(A)
    A.run_reserve(NREC, NSTEPS)
    upload_series(A, rec)
    A.run(DT, sch, st.RUN_HISTORY)
    B = device(base)
    B.set_graph(True)
    _history(B)
    B.run_reserve(NREC, NSTEPS)
    upload_series(B, rec)
    B.run(DT, sch[:N], st.RUN_HISTORY)
    img = B.restart_save()
    B.close()
    Cx, ids_c = _fresh(base, graph=True)
    Cx.run_reserve(NREC, NSTEPS)
    Cx.restart_load(img)
    upload_series(Cx, rec)
    Cx.run(DT, sch[N:], st.RUN_HISTORY)
    _assert_same(_snapshot(A, ids), _snapshot(Cx, ids_c), skip=st.SERIES_FORCING + st.SERIES_PHENOLOGY)
    A.close()
    Cx.close()


def test_decomposition_change(base):
    """Two halves save with their gcol0; merged, then cut into three uneven blocks, each loaded and continued: the one-context
    run, column for column (fields and column history)."""
    n = base[0]["snl"].shape[0]
    rec = base[5]
    sch = schedule()
    A = device(base)
    ids = _history(A, gridded=False)
    stepwise(A, rec, sch, st.RUN_HISTORY)
    want = _snapshot(A, ids)
    A.close()
    halves = [(0, 1400), (1400, n - 1400)]
    imgs = []
    for c0, m in halves:
        half = device(_sub(base, c0, m))
        _history(half, gridded=False)
        stepwise(half, _sub(base, c0, m)[5], sch[:N], st.RUN_HISTORY)
        imgs.append(half.restart_save(c0))
        half.close()
    full = R.merge(imgs[::-1])
    for c0, m in [(0, 517), (517, 1999), (2516, n - 2516)]:
        part = R.slice(full, c0, m)
        sub = _sub(base, c0, m)
        D, ids_d = _fresh(sub, gridded=False)
        D.restart_load(part, c0)
        stepwise(D, sub[5], sch[N:], st.RUN_HISTORY)
        got = _snapshot(D, ids_d)
        for k in D.fields:
            assert same(got[k], want[k][c0:c0 + m]), k
        for x, y in zip(got["hist"], want["hist"]):
            assert same(x, y[c0:c0 + m])
        assert got["counts"] == want["counts"]
        D.close()


def test_image_contents(base):
    """Field sections equal elmk_download bit for bit; the device's checksums equal restart.py's; the image holds exactly the
    PROGNOSTIC and SURFACE fields."""
    D = device(base)
    stepwise(D, base[5], schedule()[:2])
    img = D.restart_save(gcol0=12345)
    assert img.size == D.restart_size()
    R.verify(img)
    secs = R.field_sections(img)
    want = {fid for name, (fid, _, _) in D.fields.items() if st.field_class(name) in IMAGE_CLASSES}
    assert set(secs) == want
    for name, (fid, nlev, dt) in D.fields.items():
        if fid in secs:
            got = secs[fid]
            ref = D[name].reshape(D.ncols, nlev).T
            assert same(got, np.ascontiguousarray(ref, dtype=got.dtype)), name
    D.close()


def test_refusals_leave_the_context_as_it_was(base):
    rec = base[5]
    sch = schedule()
    B = device(base)
    _history(B)
    stepwise(B, rec, sch[:N], st.RUN_HISTORY)
    img = B.restart_save()
    B.close()
    D, ids = _fresh(base)
    D.restart_load(img)
    before = _snapshot(D, ids)
    p = R.parse(img)
    snl_id = D.fields["snl"][0]
    snl_sec = [s for s in p["sections"] if int(s["kind"]) == R.FIELD and int(s["id"]) == snl_id][0]

    bad = {}
    b = img.copy()
    b[int(p["sections"][3]["offset"]) + 17] ^= 0x10
    bad["data byte"] = (b, 0)
    bad["truncated"] = (img[:img.size - 300].copy(), 0)
    bad["gcol0"] = (img, 5)
    h = p["header"].copy()
    h["schema_hash"] ^= 1
    bad["schema"] = (R.build(h, p["entries"], p["sections"], p["data"]), 0)
    bad["magic"] = (np.concatenate([np.frombuffer(b"XXXXXXXX", np.uint8), img[8:]]), 0)
    data = [d.copy() for d in p["data"]]
    sec = p["sections"].copy()
    i = list(p["sections"]["offset"]).index(snl_sec["offset"])
    data[i][0, 10] = 6
    sec[i]["checksum"] = R.checksum(data[i], 0)
    bad["snl range"] = (R.build(p["header"], p["entries"], sec, data), 0)
    for what, (b, g0) in bad.items():
        with pytest.raises(L.ElmkError):
            D.restart_load(b, g0)
        _assert_same(before, _snapshot(D, ids))
    # another ncols
    E = device(_sub(base, 0, 2000))
    _history(E)
    with pytest.raises(L.ElmkError):
        E.restart_load(img)
    E.close()
    # another history table
    E = device(base)
    E.history_add(0, "t_grnd", "avg")
    with pytest.raises(L.ElmkError):
        E.restart_load(img)
    E.close()
    # a load while the stream is being captured
    with captured(D):
        rc = D.lib.elmk_restart_load(D.ctx, 0, img.ctypes.data, img.size)
    assert rc == -1
    _assert_same(before, _snapshot(D, ids))
    # the context still gives the bits of a clean one
    Cx, ids_c = _fresh(base)
    Cx.restart_load(img)
    stepwise(D, rec, sch[N:N + 1], st.RUN_HISTORY)
    stepwise(Cx, rec, sch[N:N + 1], st.RUN_HISTORY)
    _assert_same(_snapshot(D, ids), _snapshot(Cx, ids_c))
    D.close()
    Cx.close()


# ---- the feature matrix ------------------------------------------------------------------------------------------------------------
MATRIX_N = 70  # one full wave and a partial one: the smallest shape with a tail in the piece kernel
# the optional kinds in image order: (bit of the context's mask, section kind, sections, the words a refusal names the feature by)
OPTIONAL = ((1, R.ACCUM_SECTION, 1, "accumulator entries"), (2, R.ALT_SECTION, 3, "active layer"), (4, R.HYDROLOGY_SECTION, 2, "soil hydrology"),
            (8, R.IRRIGATION_SECTION, 2, "irrigation"))
NMASK = 1 << len(OPTIONAL)
# What the library did before the host API was split, recorded once from that build, for the masks without the irrigation: per mask
# (version, image bytes, the optional section kinds after the field sections), and the (image mask, context mask) pairs that load.
MATRIX_IMAGES = {0: (1, 298240, ()), 1: (2, 299008, (3,)), 2: (3, 300544, (4, 4, 4)), 3: (3, 301568, (3, 4, 4, 4)),
                 4: (4, 299776, (5, 5)), 5: (4, 300544, (3, 5, 5)), 6: (4, 302336, (4, 4, 4, 5, 5)), 7: (4, 303104, (3, 4, 4, 4, 5, 5))}
MATRIX_LOADS = {(m, m) for m in range(8)}


def _matrix_context(inputs, mask):
    D = device(inputs)
    n = D.ncols
    D["t_grnd"] = np.full(n, 250.0 + mask)
    if mask & 1:
        D.accum_init(D.accum_add("t_grnd", "runmean", 10), np.arange(n) + 0.5 * mask, nsteps=3 + mask)
    if mask & 2:
        D.active_layer_enable()
        D.active_layer_init(np.arange(n) * 0.01 + mask, np.arange(n) * 0.02 + mask)
    if mask & 4:
        D.soil_hydrology_enable()
        D.soil_hydrology_init(np.arange(n) * 0.03 + mask, 4000.0 + np.arange(n) + mask)
    if mask & 8:
        D.irrigation_enable(np.arange(n, dtype=np.int32) * 1200 - 1)
        D.irrigation_init(np.arange(n) * 0.04 + mask, np.arange(n) * 600.0 + mask)
    return D


def restart_matrix():
    """-> ({mask: (version, bytes, optional kinds)}, {(image mask, context mask) that load}, {refused pair: message}); asserts what
    holds for every library: the codec's round trip, and that a refusal is ELMK_E_INVALID and leaves t_grnd alone."""
    inputs = _inputs(MATRIX_N, 98)
    ctx = [_matrix_context(inputs, m) for m in range(NMASK)]
    imgs = [D.restart_save() for D in ctx]
    nfield = len(R.field_sections(imgs[0]))
    images, loads, refused = {}, set(), {}
    for m, img in enumerate(imgs):
        p = R.verify(img)
        kinds = [int(k) for k in p["sections"]["kind"]]
        assert kinds[:nfield] == [R.FIELD] * nfield
        images[m] = (int(p["header"]["version"]), int(img.size), tuple(kinds[nfield:]))
        again = R.build(p["header"], p["entries"], p["sections"], p["data"], p["accum"])
        assert again.tobytes() == img.tobytes(), m
    for src, img in enumerate(imgs):
        for dst, D in enumerate(ctx):
            before = D["t_grnd"]
            rc = D.lib.elmk_restart_load(D.ctx, 0, img.ctypes.data, img.size)
            if rc == 0:
                loads.add((src, dst))
                D["t_grnd"] = before
            else:
                assert rc == -1, (src, dst, rc)  # ELMK_E_INVALID
                assert same(D["t_grnd"], before), (src, dst)
                refused[(src, dst)] = D.lib.elmk_last_error(D.ctx).decode()
    for D in ctx:
        D.close()
    return images, loads, refused


def test_feature_matrix():
    """The 16 contexts with an accumulator entry, the active layer thickness, the soil hydrology and the irrigation each off or on: every
    image has the version include/elmk.h gives it, the optional sections in the order ACCUM, ALT, HYDROLOGY, IRRIGATION and the bytes its
    section table takes at 256-byte alignment; restart.build reproduces it from restart.parse; of the 256 loads exactly those of an image
    into the context of its own features succeed, and every other one returns ELMK_E_INVALID, leaves the state as it was and names a
    feature in which image and context differ."""
    images, loads, refused = restart_matrix()
    assert sorted(images) == list(range(NMASK))
    for m in range(NMASK):
        want_kinds = tuple(kind for bit, kind, nsec, _ in OPTIONAL if m & bit for _ in range(nsec))
        want_version = max([1] + [ver for (bit, _, _, _), ver in zip(OPTIONAL, (2, 3, 4, 5)) if m & bit])
        want_bytes = RC.layout(MATRIX_N, accum=[1] * (m & 1), optional=[kind for bit, kind, _, _ in OPTIONAL[1:] if m & bit])[1]
        if m in MATRIX_IMAGES:
            assert MATRIX_IMAGES[m] == (want_version, want_bytes, want_kinds)  # the record follows include/elmk.h
            assert images[m] == MATRIX_IMAGES[m], m
        assert images[m] == (want_version, want_bytes, want_kinds), m
    assert loads == {(m, m) for m in range(NMASK)}
    assert MATRIX_LOADS == {(s, d) for s, d in loads if s < 8 and d < 8} == {(m, m) for m in range(8)}
    assert len(loads) + len(refused) == NMASK * NMASK == 256
    for (src, dst), msg in refused.items():
        words = [w for bit, _, _, w in OPTIONAL if (src ^ dst) & bit]
        assert any(w in msg for w in words), (src, dst, msg)


def test_restart_demo(tmp_path):
    """examples/restart_demo.cc builds, restarts half way through 48 steps and prints bit-identical."""
    n = 3008
    cols, scal, soil, lat, lon, rec = _inputs(n, 74, nrec=25)
    exe = build_demo("restart_demo", tmp_path)
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, demo_records(lat, lon, rec) + [("steps", schedule(48))]))
    r = run_demo(exe, tmp_path / "state.bin", tmp_path / "restart.img")
    assert "bit-identical" in r.stdout
    R.verify(R.read(tmp_path / "restart.img"))
