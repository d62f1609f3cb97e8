"""The two things a run leaves behind as evidence of its health, at their edges, against numpy:

  * the (min, max, sum) triples of the eight conservation diagnostics (k_cons_reduce1 / k_cons_reduce2 / k_cons_reduce2_run) against
    elmkernels_amd.diagnostics.reduce_min_max_sum, the host restatement of the device's order (tests/test_diagnostics_host.py holds
    the restatement to a literal per-thread loop) - as 64-bit patterns, with values the test chooses so that the order is visible;
  * the error summary (k_flag_reduce / k_flag_reduce_run): OR of the flag words and first fatal column against np.bitwise_or.reduce
    and the first index with a fatal bit.

No physics call is needed to drive either: a fresh context holds 0.0 in every field, so with fsa, eflx_lwrad_out, h2osno and snl
uploaded the eight diagnostics of k_conservation are, exactly,
    [0] h2osno  [1] h2osno  [2] h2osno where snl > 0, else 0  [3] h2osno / dt  [4] fsa  [5] eflx_lwrad_out  [6] -eflx_lwrad_out  [7] fsa
and err_flags takes a plain upload."""
import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics as dg
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests import run_cases as GR
from tests.support import words_f64

pytestmark = pytest.mark.gpu

DT = 1800.0
T = dg.CONS_NPART * dg.CONS_BLOCK  # 131072 threads of stage 1
FATAL = 0xC7FF  # ELMK_ERR_FATAL_MASK
RDS = 1 << 6  # ELMK_ERR_SNICAR_RDS (fatal)
SOFT_A, SOFT_B = 1 << 11, 1 << 20  # bits outside the fatal mask
SIZES = [1, 63, 255, 256, 257, 20000, T - 1, T, T + 1, 2 * T + 5]
SEEDS = {1: 1, 63: 11, 255: 1, 256: 5, 257: 13, 20000: 1, T - 1: 3, T: 6, T + 1: 3, 2 * T + 5: 4}  # see order_is_visible


def same_triples(got, want):
    """64-bit patterns; any NaN equals any NaN; a min or max that is a zero compares by value (the sign of a zero extreme is the one
    met first in the device's order, which the restatement shares but no caller should lean on)."""
    got, want = np.asarray(got), np.asarray(want)
    ok = (words_f64(got) == words_f64(want)) | (np.isnan(got) & np.isnan(want))
    zero = (got == 0.0) & (want == 0.0)
    zero[..., 2] = False  # the sum's bits count, zero or not
    return bool((ok | zero).all())


def wide_values(n, seed):
    """Magnitudes log-uniform over 1e-8 .. 1e+8, random signs, an eighth of the values cancelled exactly by another eighth."""
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-8.0, 8.0, n) * rng.choice([-1.0, 1.0], n)
    k = n // 8
    if k:
        i = rng.permutation(n)[:2 * k]
        x[i[k:]] = -x[i[:k]]
    return x


def chosen_inputs(n, seed, f32=False):
    v = {"fsa": wide_values(n, seed), "eflx_lwrad_out": wide_values(n, seed + 1), "h2osno": wide_values(n, seed + 2)}
    if f32:  # libelmk_f32.so stores what it is given rounded to fp32
        v = {k: a.astype(np.float32).astype(np.float64) for k, a in v.items()}
    v["snl"] = (np.arange(n) % 3 != 0).astype(np.int32)
    return v


def expected_columns(v):
    """What k_conservation makes of the chosen inputs over a state of zeros, in numpy: [n, 8]."""
    a, b, w = v["fsa"], v["eflx_lwrad_out"], v["h2osno"]
    with np.errstate(invalid="ignore"):
        return np.stack([w, w, np.where(v["snl"] > 0, w, 0.0), w / DT, a, b, -b, a], axis=1)


def restated(cols):
    return np.stack([dg.reduce_min_max_sum(cols[:, k]) for k in range(cols.shape[1])])


def evaluate_and_check(D, v, what):
    """The per-column values are the chosen ones, and the triples are their restatement, bit for bit.  -> (triples, columns)"""
    mms, cols = st.kokkos_evaluate_conservation(D, DT, per_column=True)
    assert np.array_equal(cols, expected_columns(v), equal_nan=True), what
    want = restated(cols)
    assert same_triples(mms, want), (what, mms.tolist(), want.tolist())
    return mms, cols


def order_is_visible(cols):
    """Other orders of the same additions - numpy's pairwise sum, a running sum, a running sum from the far end - each give other
    bits than the device's order in [0], [4] and [5] (h2osno, fsa, eflx_lwrad_out: three independent sets of values).  With
    magnitudes this far apart one set agrees between two orders about one time in four, so the seeds (SEEDS) are the first for which
    none does: a device sum in one of those orders could not pass in any of the three."""
    want = restated(cols)
    others = (np.sum, lambda x: np.cumsum(x)[-1], lambda x: np.cumsum(x[::-1])[-1])
    return all(words_f64(want[k, 2])[0] != words_f64(f(cols[:, k]))[0] for k in (0, 4, 5) for f in others)


def _state(n, v, lib_path=None):
    D = st.ELMState(n, lib_path=lib_path)
    for k, a in v.items():
        D.upload(k, a)
    return D


# ---- 1. the reduction against its restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_triples_equal_the_restatement(n):
    """One lane; a ragged wave; one workgroup less one lane, exactly, plus one; the size the parity test uses; the last size every
    thread sees at most one element; the first second trip; two full trips and a ragged third."""
    v = chosen_inputs(n, SEEDS[n])
    D = _state(n, v)
    mms, cols = evaluate_and_check(D, v, n)
    if n >= 63:
        assert order_is_visible(cols), n
    assert np.array_equal(mms[:, 0], cols.min(axis=0)) and np.array_equal(mms[:, 1], cols.max(axis=0))
    D.close()


def test_triples_equal_the_restatement_fp32_state_library():
    """libelmk_f32.so: the state is stored as fp32, the diagnostics scratch and the reduction are fp64 there too."""
    n = T + 1
    v = chosen_inputs(n, 2, f32=True)
    D = _state(n, v, lib_path=L.F32_LIB_PATH)
    assert D.lib.elmk_state_real_bytes() == 4
    mms, cols = evaluate_and_check(D, v, "f32")
    assert order_is_visible(cols)
    D.close()


def _stepwise_columns(D, rec, steps):
    """tests/run_cases.py's stepwise loop, keeping every step's per-column diagnostics and err_flags."""
    cons, cols, flags = [], [], []
    for p in steps:
        D.solar_geometry(DT, float(p["decday"]), int(p["doy"]))
        f = int(p["forc_slot"])
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([rec[k][f], rec[k][f + 1]], axis=1))
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([rec[k][p["month1"]], rec[k][p["month2"]]], axis=1))
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"])
        st.kokkos_init_timestep(D)
        st.advance_physics(D, DT)
        m, c = st.kokkos_evaluate_conservation(D, DT, per_column=True)
        cons.append(m)
        cols.append(c)
        flags.append((D["err_flags"], D.error_summary()))
    return cons, cols, flags


def test_run_rows_equal_the_restatement():
    """elmk_run over three steps at the first size with a second trip: every row of run_diagnostics() (k_cons_reduce2_run) is the
    restatement of that step's per-column values, which the stepwise calls of the same steps give."""
    n = T + 1
    cols, scal, soil, lat, lon, rec = GR._inputs(n, 75, nrec=4)
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    steps = GR.schedule(3)
    cons, percol, _ = _stepwise_columns(A, rec, steps)
    B.run_reserve(4, 3)
    GR.upload_series(B, rec)
    B.run(DT, steps)
    rows = B.run_diagnostics()[0]
    assert rows.shape == (3, 8, 3)
    for s in range(3):
        want = restated(percol[s])
        assert same_triples(rows[s], want), (s, rows[s].tolist(), want.tolist())
        assert same_triples(cons[s], want), s
        assert any(words_f64(want[k, 2]) != words_f64(np.sum(percol[s][:, k])) for k in range(8)), s  # the order shows in physical values too
    assert len({rows[s, 6, 2] for s in range(3)}) == 3  # the steps differ
    A.close()
    B.close()


# ---- 2. non-finite values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,where", [(257, (0, 100, 256)), (T + 1, (0, 70037, T))])
@pytest.mark.parametrize("what", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_column_shows_in_the_triples(n, where, what):
    """include/elmk.h, elmk_evaluate_conservation: a NaN in any column makes min, max and sum of that diagnostic NaN; an infinity is an
    ordinary value.  Planted in turn in column 0, in the middle of a wave, and in the last column - which at n = 131073 is the one
    column that only a second trip of the grid-stride loop reaches.  (With fmin / fmax, which drop a NaN, min and max stayed clean.)"""
    base = chosen_inputs(n, SEEDS[n])
    D = _state(n, base)
    for c in where:
        v = {k: a.copy() for k, a in base.items()}
        for k in ("fsa", "eflx_lwrad_out", "h2osno"):
            v[k][c] = what
            D.upload(k, v[k][c:c + 1], col0=c)
        v["snl"][c] = 1  # (the snow balance [2] carries h2osno only where there is snow)
        D.upload("snl", v["snl"][c:c + 1], col0=c)
        mms, cols = evaluate_and_check(D, v, (n, c))
        if np.isnan(what):
            assert np.isnan(mms).all(), (n, c, mms.tolist())
        else:
            hi = [0, 1, 2, 3, 4, 5, 7]  # +inf arrives as +inf; [6] = -eflx_lwrad_out as -inf
            assert (mms[hi, 1] == np.inf).all() and (mms[hi, 2] == np.inf).all() and np.isfinite(mms[hi, 0]).all(), (n, c, mms.tolist())
            assert mms[6, 0] == -np.inf and mms[6, 2] == -np.inf and np.isfinite(mms[6, 1])
        for k in v:  # back to the clean values
            D.upload(k, base[k][c:c + 1], col0=c)
    _, cols = evaluate_and_check(D, base, (n, "clean again"))
    assert order_is_visible(cols)
    D.close()


def test_opposite_infinities_sum_to_nan():
    n = 257
    v = chosen_inputs(n, 32)
    v["fsa"][3], v["fsa"][200] = np.inf, -np.inf
    D = _state(n, v)
    mms, _ = evaluate_and_check(D, v, "inf - inf")
    for k in (4, 7):
        assert mms[k, 0] == -np.inf and mms[k, 1] == np.inf and np.isnan(mms[k, 2])
    assert np.isfinite(mms[[0, 1, 2, 3, 5, 6]]).all()
    D.close()


# ---- 3. the error summary at its edges -----------------------------------------------------------------------------------------
def numpy_summary(flags):
    fatal = np.nonzero(flags & np.uint32(FATAL))[0]
    return int(np.bitwise_or.reduce(flags)) if flags.size else 0, int(fatal[0]) if fatal.size else -1


def summary_of(D, placed):
    """Upload flag words {column: word} over zeros and summarise: the device's answer, checked against numpy's."""
    flags = np.zeros(D.ncols, np.uint32)
    for c, w in placed.items():
        flags[c] = w
    D.upload("err_flags", flags)
    assert np.array_equal(D["err_flags"], flags)
    got = D.error_summary()
    assert got == numpy_summary(flags), (D.ncols, placed, got, numpy_summary(flags))
    return got


def test_non_fatal_bits_do_not_name_a_column():
    n = 2048 + 77
    D = st.ELMState(n)
    assert D.error_summary() == (0, -1)
    # a column with only a non-fatal bit precedes the first fatal one: not it, but its bit is in the OR
    assert summary_of(D, {5: SOFT_A, 700: RDS, 701: SOFT_B | 2}) == (SOFT_A | SOFT_B | RDS | 2, 700)
    assert summary_of(D, {0: SOFT_B, 63: SOFT_A, 64: SOFT_A, n - 1: 1 << 15}) == (SOFT_A | SOFT_B | (1 << 15), n - 1)
    # only non-fatal bits anywhere
    assert summary_of(D, {0: SOFT_A, 1000: SOFT_B, n - 1: SOFT_A}) == (SOFT_A | SOFT_B, -1)
    D.close()


@pytest.mark.parametrize("n", [1, 65, 100, 257])
def test_a_fatal_bit_at_the_edges_of_waves(n):
    """A single fatal bit in column 0, 63, 64 and n - 1 (the last lane of a wave, the first of the next, the last lane of a ragged last
    wave), each fatal bit of the mask in turn at n - 1; then clearing, and stickiness."""
    D = st.ELMState(n)
    for c in sorted({0, 63, 64, n - 1}):
        if c < n:
            assert summary_of(D, {c: RDS}) == (RDS, c)
    for b in range(32):
        if FATAL >> b & 1:
            assert summary_of(D, {n - 1: 1 << b}) == (1 << b, n - 1)
    if n > 1:  # a non-fatal bit in the last lane, a fatal one before it
        assert summary_of(D, {n - 1: SOFT_A, n - 2: 1}) == (SOFT_A | 1, n - 2)
    first = D.error_summary()
    assert D.error_summary() == first and first[0] != 0  # a second summary without clearing repeats the first
    D.clear_errors()
    assert D.error_summary() == (0, -1)
    assert not D["err_flags"].any()
    D.close()


def test_past_the_workgroup_cap():
    """n = 524288 + 300: 2048 workgroups of 256 cover 524288 columns, the last 300 are reached by a second trip only.  Nothing but the
    flags is uploaded at this size."""
    n = 2048 * 256 + 300
    D = st.ELMState(n)
    assert summary_of(D, {n - 1: RDS}) == (RDS, n - 1)
    assert summary_of(D, {n - 1: RDS, 2048 * 256 + 1: 1 << 14}) == (RDS | (1 << 14), 2048 * 256 + 1)
    # the same thread sees column 44 (first trip) and 524288 + 44 (second): the earlier one wins whichever is fatal
    assert summary_of(D, {44: SOFT_A, 2048 * 256 + 44: 2}) == (SOFT_A | 2, 2048 * 256 + 44)
    assert summary_of(D, {44: 2, 2048 * 256 + 44: 4, n - 1: SOFT_B}) == (SOFT_B | 6, 44)
    D.clear_errors()
    assert D.error_summary() == (0, -1)
    D.close()


def test_run_rows_of_the_error_summary():
    """Two runs of four steps over snow-free columns.  The first raises nothing: rows (0, -1).  Then one sunlit column's state is
    replaced by a column under one layer of snow whose grain radius lies beyond the Mie table, so that it throws in the first step of
    the second run (snow_snicar_impl.hh:76): every row of the second run carries that bit (flags are sticky) and that column.  The
    expected rows are numpy's summary of the stepwise err_flags after the same step."""
    n = 1029
    cols, scal, soil, lat, lon, rec = GR._inputs(n, 76, nrec=6, tier="A")
    snowy = synth.make_state(st.field_table(), n, tier="B", seed=76)[0]
    j = int(np.nonzero(snowy["snl"] == 1)[0][0])
    A = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    B = H.device_state(cols, scal, soil, lat=lat, lon=lon)
    steps = GR.schedule(8)
    B.run_reserve(6, 4)
    GR.upload_series(B, rec)

    def both(sl):
        _, _, flags = _stepwise_columns(A, rec, steps[sl])
        B.run(DT, steps[sl])
        _, fo, fb = B.run_diagnostics()
        assert fo.shape == fb.shape == (4,)
        for s, (words, stepwise_summary) in enumerate(flags):
            assert (int(fo[s]), int(fb[s])) == numpy_summary(words) == stepwise_summary, (s, fo, fb)
        return fo, fb

    fo, fb = both(slice(0, 4))
    assert not fo.any() and (fb == -1).all()
    # a column the sun stands over during the second run: only there SNICAR reads the grain radius
    cz = []
    for s in (4, 7):
        A.solar_geometry(DT, float(steps[s]["decday"]), int(steps[s]["doy"]))
        cz.append(A["coszen"])
    c = int(np.argmax(np.minimum(*cz)))
    assert min(cz[0][c], cz[1][c]) > 0.3 and c > 0
    for D in (A, B):
        for k, v in snowy.items():
            if k not in GR.SERIES and k != "coszen":
                D.upload(k, np.ascontiguousarray(v[j:j + 1]), col0=c)
        D.upload("snw_rds", np.full((1, 5), 5000.0), col0=c)
    fo, fb = both(slice(4, 8))
    assert ((fo & RDS) != 0).all() and (fb == c).all(), (fo, fb, c)
    A.close()
    B.close()
