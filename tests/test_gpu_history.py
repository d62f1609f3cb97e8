"""History accumulation on the device (elmk_history_*, k_history.hip): every entry against numpy applying the rules of include/elmk.h
("history") to elmk_download results taken after every step, bit for bit; the physics unchanged by accumulating; a caller's graph;
the refusals; libelmk_f32.so; the example; the ends of a column pair and of a workgroup (1 .. 1025 columns, every stored type, U32
among them, both builds) and every edge value under every op."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.run_cases import NumpyTapes
from tests.support import build_demo, captured, run_demo, same, same_nan, state_blob

pytestmark = pytest.mark.gpu

DT = 1800.0
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


def _device(n, seed, lib_path=None):
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=seed)
    return H.device_state(cols, scal, soil, lib_path=lib_path), cols


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
        assert same_nan(got, want), ref.entries[k]
        if want.ndim == 2:
            assert same_nan(D.history_read(e, layout=st.LAYOUT_SOA), want.T), ref.entries[k]
        c0, m = n // 3 + 1, n // 2 - 7
        assert same_nan(D.history_read(e, col0=c0, n=m), want[c0:c0 + m]), ref.entries[k]
        if want.ndim == 2:
            assert same_nan(D.history_read(e, col0=c0, n=m, layout=st.LAYOUT_SOA), want[c0:c0 + m].T), ref.entries[k]
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
    assert not same_nan(ref.result(ENTRIES.index((1, "t_grnd", "max"))), ref.result(ENTRIES.index((1, "t_grnd", "min"))))
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
    assert same_nan(D.history_read(e), D["t_grnd"])
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
                assert same_nan(D.history_read(e), np.full(n, want))
    for e in ids[:4]:
        assert np.isnan(D.history_read(e)).all()
    assert same_nan(D.history_read(ids[4]), np.full(n, -3.0))  # INST: the last sample, not sticky
    s = D.history_read(z)
    assert (s == 0.0).all() and np.signbit(s).all()  # -0.0 + -0.0 ... = -0.0
    assert (D.history_read(zmax) == 0.0).all()
    D.close()


OPS = ("avg", "sum", "max", "min", "inst")
# every op on every stored type: F64 with one level and with 20, I32, U8 and U32 (err_flags), over three tapes
END_ENTRIES = [(k % 3, f, op) for k, (f, op) in
               enumerate((f, op) for f in ("t_grnd", "t_soisno", "snl", "veg_active", "err_flags") for op in OPS)]


@pytest.mark.parametrize("ncols,lib_path", [(n, None) for n in (1, 2, 3, 511, 512, 513, 1025)] + [(n, L.F32_LIB_PATH) for n in (1, 513, 1025)],
                         ids=lambda v: "f32" if v == L.F32_LIB_PATH else "f64" if v is None else None)
def test_pair_and_workgroup_ends(ncols, lib_path):
    """k_hist_accumulate takes two columns per thread and 512 per workgroup: one column (half a pair), a pair, a pair and a half, a
    workgroup less one column, a workgroup, a workgroup and one column, two and one.  Three accumulates of directly uploaded values
    against numpy's fold of the downloads, whole and for the last column alone; in both builds at 1, 513 and 1025."""
    D = st.ELMState(ncols, lib_path=lib_path)
    ids = [D.history_add(*e) for e in END_ENTRIES]
    ref = NumpyTapes(END_ENTRIES)
    names = sorted({f for _, f, _ in END_ENTRIES})
    rng = np.random.default_rng(40 + ncols)
    for _ in range(3):
        D["t_grnd"] = rng.standard_normal(ncols) * 300.0
        D["t_soisno"] = rng.standard_normal((ncols, D.fields["t_soisno"][1])) * 300.0
        D["snl"] = rng.integers(0, 6, ncols).astype(np.int32)
        D["veg_active"] = rng.integers(0, 256, ncols).astype(np.uint8)
        flags = rng.integers(0, 1 << 32, ncols, dtype=np.uint64).astype(np.uint32)
        flags[-1] |= np.uint32(1 << 31)  # (the last column, the one read alone: above 2^31)
        D["err_flags"] = flags
        assert same(D["err_flags"], flags)
        D.history_accumulate()
        ref.fold({k: D[k] for k in names})
    for k, e in enumerate(ids):
        want = ref.result(k)
        assert same_nan(D.history_read(e), want), (ncols, END_ENTRIES[k])
        assert same_nan(D.history_read(e, col0=ncols - 1, n=1), want[ncols - 1:]), (ncols, END_ENTRIES[k], "the last column")
        if want.ndim == 2:
            assert same_nan(D.history_read(e, col0=ncols - 1, n=1, layout=st.LAYOUT_SOA), want[ncols - 1:].T), (ncols, END_ENTRIES[k])
    assert [D.history_count(t) for t in range(3)] == [3, 3, 3]
    u = D.history_read(ids[[(f, op) for _, f, op in END_ENTRIES].index(("err_flags", "max"))])
    assert u[-1] >= 2.0 ** 31  # widened as unsigned
    D.close()


NAN, INF, BIG = float("nan"), float("inf"), 1.7976931348623157e308
# three samples per class of column (column c is of class c % 10); class 9 holds ordinary numbers
EDGE_SAMPLES = ((INF, -INF, 1.0),  # 0: SUM and AVG meet +inf then -inf: NaN from then on
                (1e300, 1e300, 1e300),  # 1: 1e300 + 1e300 is 2e300 in fp64 (the largest fp64 is 1.8e308) ...
                (BIG, BIG, -1.0),  # 2: ... the sum that overflows: +inf, and stays
                (-INF, -INF, -INF),  # 3: MAX's initial value as a sample leaves it; MIN takes it
                (INF, INF, INF),  # 4: the mirror
                (-0.0, 0.0, -0.0),  # 5: MAX and MIN keep the first zero ...
                (0.0, -0.0, 0.0),  # 6: ... in either order
                (NAN, 2.5, -3.0),  # 7: a NaN sticks to SUM, AVG, MAX and MIN; INST takes the number after it
                (5e-324, 5e-324, 5e-324))  # 8: subnormal sums are exact


def test_edge_values_by_op():
    """1000 columns, every edge value in columns of its own, three samples ordered as EDGE_SAMPLES says; against numpy's fold and,
    for the cases named there, by value."""
    n = 1000
    D = st.ELMState(n)
    entries = [(0, "t_grnd", op) for op in OPS]
    ids = [D.history_add(*e) for e in entries]
    ref = NumpyTapes(entries)
    cls = np.arange(n) % 10
    rng = np.random.default_rng(45)
    for k in range(3):
        v = rng.standard_normal(n) * 300.0
        for c, samples in enumerate(EDGE_SAMPLES):
            v[cls == c] = samples[k]
        D["t_grnd"] = v
        assert same_nan(D["t_grnd"], v)
        D.history_accumulate()
        with np.errstate(all="ignore"):
            ref.fold({"t_grnd": D["t_grnd"]})
    got = {}
    for k, e in enumerate(ids):
        got[OPS[k]] = D.history_read(e)
        assert same_nan(got[OPS[k]], ref.result(k)), OPS[k]

    def of(op, c):
        return got[op][cls == c]

    def all_bits(a, v):
        return same(a, np.full(a.shape, v))

    assert np.isnan(of("sum", 0)).all() and np.isnan(of("avg", 0)).all() and all_bits(of("max", 0), INF) and all_bits(of("min", 0), -INF)
    assert all_bits(of("sum", 1), 1e300 + 1e300 + 1e300) and np.isfinite(of("avg", 1)).all()
    assert all_bits(of("sum", 2), INF) and all_bits(of("avg", 2), INF) and all_bits(of("max", 2), BIG) and all_bits(of("min", 2), -1.0)
    assert all_bits(of("max", 3), -INF) and all_bits(of("min", 3), -INF) and all_bits(of("sum", 3), -INF)
    assert all_bits(of("max", 4), INF) and all_bits(of("min", 4), INF) and all_bits(of("inst", 4), INF)
    assert all_bits(of("max", 5), -0.0) and all_bits(of("min", 5), -0.0)  # the first zero stays
    assert all_bits(of("max", 6), 0.0) and all_bits(of("min", 6), 0.0)
    assert all_bits(of("sum", 5), 0.0) and all_bits(of("sum", 6), 0.0)  # -0.0 + -0.0 + +0.0 ... = +0.0
    for op in ("sum", "avg", "max", "min"):
        assert np.isnan(of(op, 7)).all(), op
    assert all_bits(of("inst", 7), -3.0)  # not sticky
    assert all_bits(of("sum", 8), 1.5e-323) and all_bits(of("avg", 8), 5e-324) and all_bits(of("max", 8), 5e-324)
    assert np.isfinite(np.stack([got[op][cls == 9] for op in OPS])).all()
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


def test_accumulate_inside_a_callers_graph():
    """elmk_history_accumulate captured alone into a caller's graph on the caller's one stream (no fork: elmk_set_stream) and
    replayed N times: count N, sums equal to N additions bit for bit.  history_add is refused while the stream is being captured."""
    n, N = 5000, 9
    D = st.ELMState(n)
    rng = np.random.default_rng(8)
    vals = {k: rng.standard_normal((n,) if D.fields[k][1] == 1 else (n, D.fields[k][1])) * 300 for k in ("t_grnd", "t_soisno")}
    for k, v in vals.items():
        D[k] = v
    es = D.history_add(0, "t_grnd", "sum")
    ea = D.history_add(0, "t_soisno", "avg")
    emx = D.history_add(1, "t_soisno", "max")
    with captured(D) as cap:
        rc_acc = D.lib.elmk_history_accumulate(D.ctx)
        rc_add = D.lib.elmk_history_add(D.ctx, 2, D.fields["t_grnd"][0], st.HIST_SUM)
        cap.end()
        assert rc_acc == 0 and rc_add == -1
        cap.replay(N)
        assert D.history_count(0) == N and D.history_count(1) == N
        acc1, acc2 = np.full(n, -0.0), np.full(vals["t_soisno"].shape, -0.0)
        for _ in range(N):
            acc1 = acc1 + vals["t_grnd"]
            acc2 = acc2 + vals["t_soisno"]
        assert same_nan(D.history_read(es), acc1)
        assert same_nan(D.history_read(ea), acc2 / float(N))
        assert same_nan(D.history_read(emx), vals["t_soisno"])
    D.close()


def test_an_exception_inside_a_capture_leaves_the_context_usable():
    """A Python exception raised in the body of support.captured after one captured call: the capture is ended and the context is
    back on its own stream, so it synchronises, downloads what it held, and an accumulate outside any capture counts one sample."""
    n = 64
    D = st.ELMState(n)
    D["t_grnd"] = 250.0 + np.arange(n, dtype=np.float64)
    e = D.history_add(0, "t_grnd", "sum")
    before = D["t_grnd"]
    with pytest.raises(RuntimeError, match="in the body"):
        with captured(D):
            D.history_accumulate()
            raise RuntimeError("in the body")
    D.sync()
    assert same(D["t_grnd"], before)
    assert D.history_count(0) == 0  # captured, never run
    D.history_accumulate()
    assert D.history_count(0) == 1 and same_nan(D.history_read(e), before)
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
    assert same_nan(D.history_read(e0), np.full(n, 5.0)) and same_nan(D.history_read(1), np.full(n, 3.0))
    assert D.history_count(0) == 2 and D.history_count(1) == 1
    with pytest.raises(L.ElmkError):
        D.history_read(e0, col0=n - 10, n=11)
    D.history_clear()
    assert D.history_count(0) == 0
    assert D.history_add(0, "t_grnd", "avg") == 0  # ids start again, the tape is clean
    D.history_accumulate()
    assert same_nan(D.history_read(0), np.full(n, 3.0))
    # the state was never written
    assert same_nan(D["t_grnd"], np.full(n, 3.0))
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
    n, nsteps = 3008, 12
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=33)
    S = H.oracle_state(cols, scal, soil)
    exe = build_demo("history_demo", tmp_path)
    e = np.random.default_rng(3).random(8)
    wt1, wt2 = 1.0 - e, e
    (tmp_path / "state.bin").write_bytes(state_blob(S, DT, [("forc_wt1", wt1), ("forc_wt2", wt2), ("month_wt", np.array([0.3, 0.7]))]))
    r = run_demo(exe, tmp_path / "state.bin", nsteps, tmp_path / "out.bin")
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
        assert same_nan(got[k], ref.result(k)), ref.entries[k]
    D.close()
