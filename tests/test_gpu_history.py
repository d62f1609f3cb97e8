"""History accumulation on the device (elmk_history_*, k_history.hip): every entry against numpy applying the rules of include/elmk.h
("history") to elmk_download results taken after every step, bit for bit; the physics unchanged by accumulating; a caller's graph;
the refusals; libelmk_f32.so; the example."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

DT = 1800.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HGT = ("forc_hgt_u_patch", "forc_hgt_t_patch", "forc_hgt_q_patch")

# (tape, field, op): every op on F64 with one level and with 20 levels, I32 (snl) and U8 (veg_active), over three tapes
ENTRIES = [
    (0, "t_grnd", "avg"), (0, "eflx_sh_tot", "sum"), (0, "t_soisno", "avg"), (0, "snl", "avg"), (0, "veg_active", "avg"),
    (0, "qflx_evap_tot", "inst"), (0, "h2osoi_liq", "min"),
    (1, "t_grnd", "max"), (1, "t_grnd", "min"), (1, "h2osoi_liq", "max"), (1, "snl", "min"), (1, "h2osoi_liq", "sum"),
    (1, "veg_active", "max"), (1, "eflx_sh_tot", "avg"),
    (2, "t_soisno", "inst"), (2, "eflx_sh_tot", "min"), (2, "qflx_evap_tot", "sum"), (2, "snl", "inst"), (2, "veg_active", "min"),
    (2, "qflx_evap_tot", "max"), (2, "t_soisno", "max"), (2, "snl", "max"), (2, "veg_active", "sum"), (2, "qflx_evap_tot", "avg"),
]


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


class NumpyTapes:
    """The contract of include/elmk.h applied on the host: fp64 accumulators, one fold per sample in step order."""

    INIT = {"avg": -0.0, "sum": -0.0, "max": -np.inf, "min": np.inf, "inst": np.nan}

    def __init__(self, entries):
        self.entries = entries
        self.acc = [None] * len(entries)
        self.count = [0] * st.HIST_MAX_TAPES

    def reset(self, tape):
        self.count[tape] = 0
        for k, (t, _, _) in enumerate(self.entries):
            if t == tape:
                self.acc[k] = None

    def fold(self, values):
        for k, (t, name, op) in enumerate(self.entries):
            v = values[name].astype(np.float64)
            a = self.acc[k] if self.acc[k] is not None else np.full(v.shape, self.INIT[op])
            if op in ("avg", "sum"):
                a = a + v
            elif op == "max":
                a = np.where((v > a) | (v != v), v, a)
            elif op == "min":
                a = np.where((v < a) | (v != v), v, a)
            else:
                a = v.copy()
            self.acc[k] = a
        for t in {t for t, _, _ in self.entries}:
            self.count[t] += 1

    def result(self, k):
        t, _, op = self.entries[k]
        return self.acc[k] / float(self.count[t]) if op == "avg" else self.acc[k]


def _device(n, seed, lib_path=None):
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=seed)
    D = st.ELMState(n, lib_path=lib_path)
    pft, optics = synth.load_params()
    D.set_pft(pft)
    D.set_snicar(optics)
    D.set_soilcolor(soil["albsat"], soil["albdry"])
    D.set_land(**synth.TEST_LAND)
    D.set_scalars(**scal)
    D.set_snow_age_tables(synth.snow_age_tables())
    for k, v in cols.items():
        D.upload(k, v)
    return D, cols


def _step(D, cols):
    for k in HGT:  # the driver puts the forcing heights back every step (atm_physics_impl.hh:197-203)
        D[k] = cols[k]
    st.kokkos_init_timestep(D)
    st.advance_physics(D, DT)


def _check_all(D, ref, ids):
    n = D.ncols
    for k, e in enumerate(ids):
        want = ref.result(k)
        got = D.history_read(e)
        assert same(got, want), ref.entries[k]
        if want.ndim == 2:
            assert same(D.history_read(e, layout=st.LAYOUT_SOA), want.T), ref.entries[k]
        c0, m = n // 3 + 1, n // 2 - 7
        assert same(D.history_read(e, col0=c0, n=m), want[c0:c0 + m]), ref.entries[k]
        if want.ndim == 2:
            assert same(D.history_read(e, col0=c0, n=m, layout=st.LAYOUT_SOA), want[c0:c0 + m].T), ref.entries[k]
    for t in range(st.HIST_MAX_TAPES):
        assert D.history_count(t) == ref.count[t], t


def _run(n, seed, nsteps, resets=None, lib_path=None):
    D, cols = _device(n, seed, lib_path)
    assert D.level_stride != n
    ids = [D.history_add(t, name, op) for t, name, op in ENTRIES]
    assert ids == list(range(len(ENTRIES)))
    ref = NumpyTapes(ENTRIES)
    names = sorted({name for _, name, _ in ENTRIES})
    for s in range(nsteps):
        _step(D, cols)
        D.history_accumulate()
        ref.fold({k: D[k] for k in names})
        for t in (resets or {}).get(s, ()):
            D.history_reset(t)
            ref.reset(t)
    _check_all(D, ref, ids)
    return D, ref


def test_every_op_and_dtype_bitwise_against_numpy_over_a_real_run():
    """Seven steps of elmk_advance_physics at 4 133 columns (level stride 4 160): 24 entries on three tapes, read in both layouts,
    whole and in part, equal to numpy's fold of the per-step downloads bit for bit; the counts are the number of steps."""
    D, ref = _run(4133, 14, 7)
    assert ref.count[:3] == [7, 7, 7] and ref.count[3] == 0
    # the run moved the snow mesh and the fluxes: the extremes differ from the averages somewhere
    assert not same(ref.result(ENTRIES.index((1, "t_grnd", "max"))), ref.result(ENTRIES.index((1, "t_grnd", "min"))))
    D.close()


def test_reset_in_the_middle_of_a_run():
    """Tape 0 reset after the fourth step while tapes 1 and 2 keep going: all three match numpy; a reset tape accepts new entries."""
    D, ref = _run(2111, 15, 7, resets={3: [0]})
    assert ref.count[:3] == [3, 7, 7]
    with pytest.raises(L.ElmkError):
        D.history_add(1, "t_grnd", "avg")  # tape 1 holds samples
    D.history_reset(2)
    e = D.history_add(2, "t_grnd", "sum")
    D.history_accumulate()
    assert D.history_count(2) == 1 and D.history_count(0) == 4
    assert same(D.history_read(e), D["t_grnd"])
    D.close()


def test_nan_sticks_and_signed_zero_survives():
    n = 1000
    D = st.ELMState(n)
    ops = ["max", "min", "sum", "avg", "inst"]
    ids = [D.history_add(0, "t_grnd", op) for op in ops]
    z = D.history_add(0, "eflx_sh_tot", "sum")
    zmax = D.history_add(0, "eflx_sh_tot", "max")
    D.fill("eflx_sh_tot", -0.0)
    for k, v in enumerate([1.5, float("nan"), 2.5, -3.0]):
        D.fill("t_grnd", v)
        D.history_accumulate()
        if k == 0:
            for e, want in zip(ids, [1.5, 1.5, 1.5, 1.5, 1.5]):
                assert same(D.history_read(e), np.full(n, want))
    for e in ids[:4]:
        assert np.isnan(D.history_read(e)).all()
    assert same(D.history_read(ids[4]), np.full(n, -3.0))  # INST: the last sample, not sticky
    s = D.history_read(z)
    assert (s == 0.0).all() and np.signbit(s).all()  # -0.0 + -0.0 ... = -0.0
    assert (D.history_read(zmax) == 0.0).all()
    D.close()


@pytest.mark.parametrize("graph", [False, True])
def test_physics_is_untouched_by_accumulating(graph):
    """The same five steps with and without accumulation give every state field bit-identical, graph on and off."""
    n = 3001
    A, cols = _device(n, 16)
    B, _ = _device(n, 16)
    for D in (A, B):
        D.set_graph(graph)
    for t, name, op in ENTRIES:
        A.history_add(t, name, op)
    for s in range(5):
        _step(A, cols)
        A.history_accumulate()
        _step(B, cols)
    for name in A.fields:
        assert np.array_equal(A[name].view(np.uint8), B[name].view(np.uint8)), name
    assert A.history_count(0) == 5
    A.close()
    B.close()


def _hip_runtime():
    """The HIP runtime this process already uses (loaded by libelmk): the same instance, so streams and graphs are shared."""
    import ctypes as C

    L.load()
    path = next((ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln), None)
    assert path, "libamdhip64 is not loaded"
    hip = C.CDLL(path)
    P = C.c_void_p
    for name, args in (("hipStreamCreateWithFlags", [C.POINTER(P), C.c_uint]), ("hipStreamBeginCapture", [P, C.c_int]),
                       ("hipStreamEndCapture", [P, C.POINTER(P)]), ("hipGraphInstantiate", [C.POINTER(P), P, P, P, C.c_size_t]),
                       ("hipGraphLaunch", [P, P]), ("hipStreamSynchronize", [P]), ("hipGraphExecDestroy", [P]),
                       ("hipGraphDestroy", [P]), ("hipStreamDestroy", [P])):
        getattr(hip, name).argtypes = args
        getattr(hip, name).restype = C.c_int
    return hip


def test_accumulate_inside_a_callers_graph():
    """elmk_history_accumulate captured alone into a caller's graph on the caller's one stream (no fork: elmk_set_stream) and
    replayed N times: count N, sums equal to N additions bit for bit.  history_add is refused while the stream is being captured."""
    import ctypes as C

    hip = _hip_runtime()
    n, N = 5000, 9
    D = st.ELMState(n)
    rng = np.random.default_rng(8)
    vals = {k: rng.standard_normal((n,) if D.fields[k][1] == 1 else (n, D.fields[k][1])) * 300 for k in ("t_grnd", "t_soisno")}
    for k, v in vals.items():
        D[k] = v
    es = D.history_add(0, "t_grnd", "sum")
    ea = D.history_add(0, "t_soisno", "avg")
    emx = D.history_add(1, "t_soisno", "max")
    s, graph, exe = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0  # hipStreamNonBlocking
    D.set_stream(s.value)
    assert hip.hipStreamBeginCapture(s, 1) == 0  # hipStreamCaptureModeThreadLocal
    rc_acc = D.lib.elmk_history_accumulate(D.ctx)
    rc_add = D.lib.elmk_history_add(D.ctx, 2, D.fields["t_grnd"][0], st.HIST_SUM)
    assert hip.hipStreamEndCapture(s, C.byref(graph)) == 0
    assert rc_acc == 0 and rc_add == -1
    assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
    for _ in range(N):
        assert hip.hipGraphLaunch(exe, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    assert D.history_count(0) == N and D.history_count(1) == N
    acc1, acc2 = np.full(n, -0.0), np.full(vals["t_soisno"].shape, -0.0)
    for _ in range(N):
        acc1 = acc1 + vals["t_grnd"]
        acc2 = acc2 + vals["t_soisno"]
    assert same(D.history_read(es), acc1)
    assert same(D.history_read(ea), acc2 / float(N))
    assert same(D.history_read(emx), vals["t_soisno"])
    D.set_stream(None)
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    hip.hipStreamDestroy(s)
    D.close()


def test_refusals_leave_the_context_working():
    n = 777
    D = st.ELMState(n)
    D.fill("t_grnd", 2.0)
    nf = D.lib.elmk_num_fields()
    bad = [(0, -1, st.HIST_AVG), (0, nf, st.HIST_AVG), (0, 0, -1), (0, 0, 5), (-1, 0, 0), (st.HIST_MAX_TAPES, 0, 0)]
    for tape, field, op in bad:
        assert D.lib.elmk_history_add(D.ctx, tape, field, op) == -1, (tape, field, op)
    with pytest.raises(L.ElmkError):
        D.history_read(0)  # no entry
    e0 = D.history_add(0, "t_grnd", "sum")
    assert e0 == 0
    with pytest.raises(L.ElmkError):
        D.history_read(e0)  # the tape holds no samples
    D.history_accumulate()
    with pytest.raises(L.ElmkError):
        D.history_add(0, "t_grnd", "max")  # the tape holds samples
    for k in range(1, st.HIST_MAX_ENTRIES):
        assert D.history_add(1 + k % 3, "t_grnd", "max") == k
    with pytest.raises(L.ElmkError):
        D.history_add(1, "t_grnd", "max")  # the 65th entry
    with pytest.raises(L.ElmkError):
        D.history_read(1)  # tape 2 is empty
    D.fill("t_grnd", 3.0)
    D.history_accumulate()
    assert same(D.history_read(e0), np.full(n, 5.0)) and same(D.history_read(1), np.full(n, 3.0))
    assert D.history_count(0) == 2 and D.history_count(1) == 1
    with pytest.raises(L.ElmkError):
        D.history_read(e0, col0=n - 10, n=11)
    D.history_clear()
    assert D.history_count(0) == 0
    assert D.history_add(0, "t_grnd", "avg") == 0  # ids start again, the tape is clean
    D.history_accumulate()
    assert same(D.history_read(0), np.full(n, 3.0))
    # the state was never written
    assert same(D["t_grnd"], np.full(n, 3.0))
    D.close()


def test_fp32_state_library():
    """libelmk_f32.so: the same run at a smaller size, against numpy's fold of the widened values that library downloads."""
    D, ref = _run(1029, 17, 4, lib_path=L.F32_LIB_PATH)
    assert D.lib.elmk_state_real_bytes() == 4
    t = D["t_grnd"]
    assert np.array_equal(t, t.astype(np.float32).astype(np.float64))
    D.close()


def test_history_demo_runs(tmp_path):
    """examples/history_demo.cc compiles against include/ and libelmk; its tapes equal numpy's fold of the same run's downloads."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    n, nsteps = 3008, 12
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=33)
    S = H.oracle_state(cols, scal, soil)
    libdir = os.path.dirname(L.LIB_PATH)
    exe = str(tmp_path / "history_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "history_demo.cc"), "-L" + libdir, "-lelmk", "-Wl,-rpath," + libdir, "-o", exe])
    e = np.random.default_rng(3).random(8)
    wt1, wt2 = 1.0 - e, e
    blob = [struct.pack("<q", n)]

    def rec(name, kind, arr):
        a = np.ascontiguousarray(arr)
        blob.append(name.encode().ljust(32, b"\0") + struct.pack("<iq", kind, a.nbytes) + a.tobytes())

    for k, v in S.fields.items():
        if k != "err_flags":
            rec(k, 0, v)
    sc = S.scalars
    rec("land", 1, np.array([sc["ltype"], sc["ctype"], sc["vtype"], sc["urbpoi"], sc["lakpoi"]], np.int32))
    rec("scalars", 1, np.array([sc["dewmx"], sc["oldfflag"], sc["dayl"], sc["max_dayl"], DT], np.float64))
    for k in ("pft_psn", "pft_alb", "z0mr", "displar", "albsat", "albdry"):
        rec(k, 1, getattr(S, k))
    for i, name in enumerate(L.SNICAR_NAMES):
        rec(f"snicar/{i}", 1, S.snicar[name])
    rec("age_tau", 1, S.snowage[0])
    rec("age_kappa", 1, S.snowage[1])
    rec("age_drdt0", 1, S.snowage[2])
    rec("forc_wt1", 1, wt1)
    rec("forc_wt2", 1, wt2)
    rec("month_wt", 1, np.array([0.3, 0.7]))
    (tmp_path / "state.bin").write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(tmp_path / "state.bin"), str(nsteps), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "history over 12 steps" in r.stdout, r.stdout
    # the same run through the Python layer, downloading after every step
    D = H.device_state(cols, scal, soil)
    for k, v in S.fields.items():
        if k != "err_flags":
            D[k] = v
    avg = ["eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "eflx_soil_grnd", "fsa", "eflx_lwrad_out"]
    ref = NumpyTapes([(0, k, "avg") for k in avg] + [(1, "t_grnd", "max"), (1, "t_grnd", "min")])
    for _ in range(nsteps):
        st.compute_phenology(D, 0.3, 0.7)
        st.get_forcing(D, wt1, wt2, False)
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        ref.fold({k: D[k] for k in avg + ["t_grnd"]})
    raw = (tmp_path / "out.bin").read_bytes()
    got = np.frombuffer(raw, np.float64, 8 * n).reshape(8, n)
    counts = np.frombuffer(raw, np.int64, 2, 8 * n * 8)
    assert list(counts) == [nsteps, nsteps]
    for k in range(8):
        assert same(got[k], ref.result(k)), ref.entries[k]
    D.close()
