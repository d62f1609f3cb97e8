"""Accumulated fields on the device (include/elmk.h "accumulated fields"): k_accum_update against the numpy restatement
(elmkernels_amd/accum.py) bit for bit in both builds, t10 fed back through elmk_run against the loop with a host round trip per
step, seeding, exact restarts (also across a change of decomposition), every refusal, and the demo."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import accum
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests import helpers as H
from tests.run_cases import DT, NREC, NSTEPS, SERIES, _inputs, demo_records, device, schedule, stepwise, upload_series
from tests.support import bits, build_demo, captured, run_demo, same, same_nan, state_blob

pytestmark = pytest.mark.gpu

N = NSTEPS // 2
P10 = 4  # steps of the t10 window in the run tests: saturates inside the 12 steps
# (source, kind, period, destination): one entry of each kind with P in {4, 10}; 1 and 20 levels, fp64 and int32 sources
ENTRIES = [("t_ref2m", accum.RUNMEAN, 4, "t10"), ("t_soisno", accum.RUNMEAN, 10, "csol"), ("t_ref2m", accum.TIMEAVG, 4, "n_melt"),
           ("t_soisno", accum.TIMEAVG, 10, None), ("t_ref2m", accum.RUNACCUM, 4, "micro_sigma"), ("snl", accum.RUNACCUM, 10, None)]


def _samples(n, step, rng):
    """t_ref2m, t_soisno, snl of one update: -0.0, a NaN column, a NaN sample, the RUNACCUM reset value and values that reach its
    upper clamp; with one column the patterns come by step."""
    t = 280.0 + 15.0 * rng.standard_normal(n)
    c = np.arange(n) % 8
    if n > 1:
        if step % 3 == 0:
            t[c == 1] = -0.0
        t[c == 2] = np.nan
        if step % 7 == 3:
            t[c == 3] = -99999.0
        if step == 13:
            t[c == 5] = np.nan
        t[c == 7] = 30000.0
    else:
        if step % 5 == 1:
            t[:] = -0.0
        if step in (3, 17):
            t[:] = -99999.0
        if step == 13:
            t[:] = np.nan
        if 8 <= step <= 11:
            t[:] = 40000.0
    soi = 270.0 + 10.0 * rng.standard_normal((n, 20))
    soi[::3, 4] = -0.0
    snl = rng.integers(0, 6, n).astype(np.int32)
    return {"t_ref2m": t, "t_soisno": soi, "snl": snl}


def _soa(a):
    """A downloaded field as the accumulator's [nlev, n] (or [n]) float64 samples."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.T if a.ndim == 2 else a).astype(np.float64)


@pytest.mark.parametrize("n", [1, 193])
@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_update_equals_the_restatement(n, lib_path):
    """25 updates of six entries from fresh samples; after every one val, the count and the destination against accum.update.  The
    samples are what the device holds (downloaded: rounded to fp32 in the fp32-state build), val is fp64 in both builds."""
    D = st.ELMState(n, lib_path=lib_path)
    assert D.level_stride == 64 * ((n + 63) // 64) and D.level_stride != n
    f32 = D.lib.elmk_state_real_bytes() == 4
    before = D.device_bytes
    ids = [D.accum_add(*e) for e in ENTRIES]
    assert ids == list(range(len(ENTRIES)))
    assert D.device_bytes - before == 16 * 21 * 48 + 256 + sum(D.level_stride * 8 * (20 if e[0] == "t_soisno" else 1) for e in ENTRIES)
    rng = np.random.default_rng(7 + n)
    val = [np.zeros((20, n)) if e[0] == "t_soisno" else np.zeros(n) for e in ENTRIES]
    dst = {e[3]: D[e[3]] for e in ENTRIES if e[3]}
    for i in ids:
        got, cnt = D.accum_read(i)
        assert cnt == 0 and bits(got) == bits(val[i])
    untouched = {k: D[k] for k in D.fields if k not in dst and k not in ("t_ref2m", "t_soisno", "snl")}
    for step in range(1, 26):
        for k, v in _samples(n, step, rng).items():
            D[k] = v
        seen = {k: _soa(D[k]) for k in ("t_ref2m", "t_soisno", "snl")}
        D.accum_update()
        for i, (src, kind, period, d) in enumerate(ENTRIES):
            val[i] = accum.update(val[i], seen[src], kind, period, step)
            got, cnt = D.accum_read(i)
            assert cnt == step, (i, step)
            assert bits(got) == bits(val[i]), (i, step)
            if d:
                if accum.writes_destination(kind, period, step):
                    with np.errstate(all="ignore"):  # state precision: rounded to fp32 in the fp32-state build
                        dst[d] = (val[i].astype(np.float32).astype(np.float64) if f32 else val[i]).T
                assert bits(D[d]) == bits(np.ascontiguousarray(dst[d])), (i, step, d)
        for k in seen:  # the sources are only read
            assert bits(_soa(D[k])) == bits(seen[k]), k
    for k, v in untouched.items():
        assert same(D[k], v), k
    # the samples did what they were chosen for
    if n > 1:
        c = np.arange(n) % 8
        assert np.isnan(val[0][c == 2]).all() and np.isnan(val[0][c == 5]).all() and np.isfinite(val[0][c == 0]).all()
        assert (val[4][c == 7] == 99999.0).all() and (val[4][c == 2] == 0.0).all() and np.isfinite(val[4]).all()
    got, _ = D.accum_read(1, layout=st.LAYOUT_COL_MAJOR)
    assert got.shape == (n, 20) and bits(got) == bits(val[1].T)
    if n > 3:
        part, _ = D.accum_read(3, col0=2, n=n - 3)
        assert bits(part) == bits(val[3][:, 2:n - 1])
    D.accum_clear()
    assert D.device_bytes == before
    D.accum_update()  # nothing to do
    D.sync()
    D.close()


# ---- pair and workgroup ends, every stored type, period and count edges ----------------------------------------------------------------
def _fold_and_compare(D, entries, val, dst, seen, counts, what):
    """After one accum_update: every entry's value (whole, and the last column alone), count and destination against accum.update of
    the samples `seen`, NaNs equal.  val, dst and counts are advanced in place."""
    f32 = D.lib.elmk_state_real_bytes() == 4
    last = D.ncols - 1
    for i, (src, kind, period, d) in enumerate(entries):
        counts[i] += 1
        val[i] = accum.update(val[i], seen[src], kind, period, counts[i])
        got, cnt = D.accum_read(i)
        assert cnt == counts[i], (what, i)
        assert same_nan(got, val[i]), (what, i, entries[i])
        tail, cnt = D.accum_read(i, col0=last, n=1)
        assert cnt == counts[i] and same_nan(tail, val[i][..., last:]), (what, i, entries[i], "the last column")
        if d:
            if accum.writes_destination(kind, period, counts[i]):
                with np.errstate(all="ignore"):  # state precision: rounded to fp32 in the fp32-state build
                    dst[d] = (val[i].astype(np.float32).astype(np.float64) if f32 else val[i]).T
            assert same_nan(D[d], dst[d]), (what, i, entries[i], d)


END_SIZES = [(n, None) for n in (2, 3, 511, 512, 513, 1025)] + [(n, L.F32_LIB_PATH) for n in (513, 1025)]
end_sizes = pytest.mark.parametrize("ncols,lib_path", END_SIZES, ids=lambda v: "f32" if v == L.F32_LIB_PATH else "f64" if v is None else None)
# the three kinds on every stored type: F64 with one level and with 20, I32, U8 and U32; every kind meets every period of 1, 2, 3, 50
END_ENTRIES = [("t_grnd", accum.RUNMEAN, 3, "t10"), ("t_soisno", accum.RUNMEAN, 50, None), ("snl", accum.RUNMEAN, 2, None),
               ("veg_active", accum.RUNMEAN, 1, None), ("err_flags", accum.RUNMEAN, 50, None),
               ("t_grnd", accum.TIMEAVG, 50, None), ("t_soisno", accum.TIMEAVG, 2, "csol"), ("snl", accum.TIMEAVG, 1, None),
               ("veg_active", accum.TIMEAVG, 3, "n_melt"), ("err_flags", accum.TIMEAVG, 2, None),
               ("t_grnd", accum.RUNACCUM, 1, None), ("t_soisno", accum.RUNACCUM, 3, None), ("snl", accum.RUNACCUM, 50, None),
               ("veg_active", accum.RUNACCUM, 2, None), ("err_flags", accum.RUNACCUM, 3, "micro_sigma")]
END_SOURCES = ("t_grnd", "t_soisno", "snl", "veg_active", "err_flags")


@end_sizes
def test_pair_and_workgroup_ends(ncols, lib_path):
    """k_accum_update takes two columns per thread and 512 per workgroup: a pair, a pair and a half, a workgroup less one column, a
    workgroup (the level stride unpadded), a workgroup and one column, two and one.  Fifteen entries, seven updates from freshly
    uploaded samples; after every one the value (whole and for the last column alone), the count and the destination against
    accum.update of the samples as downloaded; in both builds at 513 and 1025."""
    assert len(END_ENTRIES) == accum.MAX_ENTRIES - 1 and {e[0] for e in END_ENTRIES} == set(END_SOURCES)
    for kind in (accum.RUNMEAN, accum.TIMEAVG, accum.RUNACCUM):
        assert {e[2] for e in END_ENTRIES if e[1] == kind} == {1, 2, 3, 50} and {e[0] for e in END_ENTRIES if e[1] == kind} == set(END_SOURCES)
    D = st.ELMState(ncols, lib_path=lib_path)
    assert (D.level_stride == ncols) == (ncols == 512)
    assert [D.accum_add(*e) for e in END_ENTRIES] == list(range(len(END_ENTRIES)))
    nlev = D.fields["t_soisno"][1]
    rng = np.random.default_rng(60 + ncols)
    for d in ("t10", "csol", "n_melt", "micro_sigma"):
        D[d] = rng.standard_normal(D[d].shape)  # what a destination holds until its entry writes it
    dst = {e[3]: D[e[3]] for e in END_ENTRIES if e[3]}
    val = [np.zeros((nlev, ncols)) if e[0] == "t_soisno" else np.zeros(ncols) for e in END_ENTRIES]
    counts = [0] * len(END_ENTRIES)
    for step in range(1, 8):
        t = rng.standard_normal(ncols) * 300.0
        t[step % ncols] = -99999.0  # RUNACCUM's reset, in a column that moves by one (either side of a pair) with every update
        t[(step + 1) % ncols] = 30000.0 * step  # ... and its upper clamp in the column beside it
        if step == 4:
            t[-1] = np.nan  # the last column, the one read alone
        D["t_grnd"] = t
        D["t_soisno"] = rng.standard_normal((ncols, nlev)) * 300.0
        D["snl"] = rng.integers(0, 6, ncols).astype(np.int32)
        D["veg_active"] = rng.integers(0, 256, ncols).astype(np.uint8)
        flags = rng.integers(0, 1 << 32, ncols, dtype=np.uint64).astype(np.uint32)
        flags[-1] |= np.uint32(1 << 31)  # (the last column: above 2^31, widened as unsigned)
        D["err_flags"] = flags
        assert same(D["err_flags"], flags)
        seen = {k: _soa(D[k]) for k in END_SOURCES}
        D.accum_update()
        _fold_and_compare(D, END_ENTRIES, val, dst, seen, counts, (ncols, step))
        for k in END_SOURCES:  # the sources are only read
            assert same_nan(_soa(D[k]), seen[k]), k
    # the samples did what they were chosen for
    assert val[4][-1] >= 2.0 ** 31 and val[9][-1] >= 2.0 ** 31  # U32 widened as unsigned (a running mean and a period's mean of the flags)
    assert np.isnan(val[0][-1]) and np.isnan(val[5][-1]) and not np.isnan(val[10]).any()  # RUNACCUM: t > 0 ? t : 0 drops a NaN
    assert (val[14] == accum.RUNACCUM_MAX).all() and (val[10] == 0.0).any() and (val[10] == accum.RUNACCUM_MAX).any()
    assert counts == [7] * len(END_ENTRIES)
    D.close()


@end_sizes
def test_seeding_past_one_workgroup(ncols, lib_path):
    """k_accum_seed at the same sizes, on one row and on twenty: accum_init without values leaves val = the destination widened and
    the count given; the next update folds into it."""
    D = st.ELMState(ncols, lib_path=lib_path)
    entries = [("t_grnd", accum.RUNMEAN, 4, "t10"), ("t_soisno", accum.RUNMEAN, 4, "csol")]
    ids = [D.accum_add(*e) for e in entries]
    nlev = D.fields["t_soisno"][1]
    rng = np.random.default_rng(70 + ncols)
    D["t10"] = 280.0 + 15.0 * rng.standard_normal(ncols)
    D["csol"] = 2.0e6 * (1.0 + rng.random((ncols, nlev)))
    D["t_grnd"] = 270.0 + 10.0 * rng.standard_normal(ncols)
    D["t_soisno"] = 270.0 + 10.0 * rng.standard_normal((ncols, nlev))
    dst = {"t10": D["t10"], "csol": D["csol"]}
    val, counts = [None, None], [0, 0]
    for i, (e, k) in enumerate(zip(ids, (9, 2))):
        D.accum_init(e, None, k)
        val[i], counts[i] = _soa(dst[entries[i][3]]), k
        got, cnt = D.accum_read(e)
        assert cnt == k and same_nan(got, val[i]) and got.any(), (ncols, e)
        tail, _ = D.accum_read(e, col0=ncols - 1, n=1)
        assert same_nan(tail, val[i][..., ncols - 1:]), (ncols, e)
    assert same_nan(D["t10"], dst["t10"]) and same_nan(D["csol"], dst["csol"])  # seeding reads the destination
    D.accum_update()
    _fold_and_compare(D, entries, val, dst, {k: _soa(D[k]) for k in ("t_grnd", "t_soisno")}, counts, (ncols, "after seeding"))
    assert counts == [10, 3]
    D.close()


RESET_SAMPLES = (-99999.0, -99999.49, -99998.51, -99999.5, -99998.5, 2.0, 1.0e6)


@pytest.mark.parametrize("lib_path", [None, L.F32_LIB_PATH], ids=["f64", "f32"])
def test_runaccum_resets_by_the_rounded_sample(lib_path):
    """RUNACCUM resets where rint(v) == -99999: -99999, -99999.49 and -99998.51 reset; the ties -99999.5 and -99998.5 round to the even
    neighbours -100000 and -99998 and do not.  Seven samples over fourteen columns, so that each stands in an even and in an odd
    column of a pair; an I32 source holds -99999 itself.  By value from a value at the upper clamp, and against accum.update."""
    n = 2 * len(RESET_SAMPLES)
    D = st.ELMState(n, lib_path=lib_path)
    entries = [("t_ref2m", accum.RUNACCUM, 4, "micro_sigma"), ("altmax_indx", accum.RUNACCUM, 4, None)]
    for e in entries:
        D.accum_add(*e)
    v = np.array(RESET_SAMPLES)[np.arange(n) % len(RESET_SAMPLES)]
    k = np.array([-99999, -99998, -100000, 7, -99999, 0, 100000], np.int32)[np.arange(n) % 7]
    assert all({int(c) % 2 for c in np.nonzero(v == s)[0]} == {0, 1} for s in RESET_SAMPLES)
    val, dst, counts = [np.zeros(n), np.zeros(n)], {"micro_sigma": D["micro_sigma"]}, [0, 0]
    for step, (t, a) in enumerate(((np.full(n, 1.0e6), np.full(n, 100000, np.int32)), (v, k), (v[::-1].copy(), k[::-1].copy()))):
        D["t_ref2m"], D["altmax_indx"] = t, a
        seen = {"t_ref2m": _soa(D["t_ref2m"]), "altmax_indx": _soa(D["altmax_indx"])}
        if step == 1:  # as stored: the fp32-state build keeps the three inexact samples on their side of the ties
            assert (np.rint(seen["t_ref2m"]) == np.rint(v)).all() and (seen["t_ref2m"][v % 0.5 == 0.0] == v[v % 0.5 == 0.0]).all()
        D.accum_update()
        _fold_and_compare(D, entries, val, dst, seen, counts, step)
        if step == 0:
            assert (val[0] == accum.RUNACCUM_MAX).all() and (val[1] == accum.RUNACCUM_MAX).all()
        if step == 1:
            reset = np.isin(v, (-99999.0, -99999.49, -99998.51))
            assert (val[0][reset] == 0.0).all() and not np.signbit(val[0][reset]).any()
            assert (val[0][v == -99998.5] == 0.5).all()  # not reset: 99999 - 99998.5
            assert (val[0][v == -99999.5] == 0.0).all()  # not reset either, but 99999 - 99999.5 < 0 is clamped to the same +0.0
            assert (val[0][v >= 2.0] == accum.RUNACCUM_MAX).all()
            assert (val[1][k == -99999] == 0.0).all() and (val[1][k == -99998] == 1.0).all() and (val[1][k == -100000] == 0.0).all()
            assert (val[1][k == 7] == accum.RUNACCUM_MAX).all()
    D.close()


def test_counts_and_periods_above_2_to_the_32():
    """AccumRow.period and the counts are 64-bit: a running mean whose window of 2^33 + 5 steps is not full after 2^33, a period average
    whose period of 2^33 steps ends with the next update (it divides by 2^33 and writes the destination) and starts anew with the one
    after; two updates against accum.update, then an image into a fresh context with the same table keeps periods, counts and values."""
    n, P0, P1 = 193, 2 ** 33 + 5, 2 ** 33
    entries = [("t_ref2m", accum.RUNMEAN, P0, "n_melt"), ("t_grnd", accum.TIMEAVG, P1, "t10")]
    rng = np.random.default_rng(91)
    seed = [280.0 + 15.0 * rng.standard_normal(n), (2.0 ** 33 - 1.0) * (270.0 + 10.0 * rng.standard_normal(n))]
    D = st.ELMState(n)
    ids = [D.accum_add(*e) for e in entries]
    D.accum_init(ids[0], seed[0], 2 ** 33)
    D.accum_init(ids[1], seed[1], 2 ** 33 - 1)
    val, counts = [seed[0].copy(), seed[1].copy()], [2 ** 33, 2 ** 33 - 1]
    assert [D.accum_read(e)[1] for e in ids] == counts
    dst = {"n_melt": D["n_melt"], "t10": D["t10"]}
    for step in range(2):
        D["t_ref2m"] = 280.0 + 15.0 * rng.standard_normal(n)
        D["t_grnd"] = 270.0 + 10.0 * rng.standard_normal(n)
        seen = {k: _soa(D[k]) for k in ("t_ref2m", "t_grnd")}
        D.accum_update()
        _fold_and_compare(D, entries, val, dst, seen, counts, step)
        if step == 0:  # the period's end: the mean of 2^33 samples of about 270 K, written to t10
            assert accum.writes_destination(accum.TIMEAVG, P1, counts[1]) and (np.abs(val[1] - 270.0) < 60.0).all() and same_nan(D["t10"], val[1])
            assert not same_nan(val[0], accum.update(seed[0], seen["t_ref2m"], accum.RUNMEAN, P0 % 2 ** 32, 1))  # (what 32-bit words would give)
        else:  # the first update of the next period: the sample itself
            assert same_nan(val[1], seen["t_grnd"]) and not same_nan(D["t10"], val[1])
    assert counts == [2 ** 33 + 2, 2 ** 33 + 1]
    img = D.restart_save()
    p = R.verify(img)
    assert [int(x) for x in p["accum"]["period"]] == [P0, P1] and [int(x) for x in p["accum"]["nsteps"]] == counts
    F = st.ELMState(n)
    for e in entries:
        F.accum_add(*e)
    F.restart_load(img)
    for i in ids:
        got, cnt = F.accum_read(i)
        assert cnt == counts[i] and same_nan(got, val[i]), i
    assert same_nan(F["t10"], D["t10"]) and same_nan(F["n_melt"], D["n_melt"])
    for X in (D, F):  # ... and both go on alike
        X["t_ref2m"], X["t_grnd"] = seen["t_ref2m"][::-1].copy(), seen["t_grnd"][::-1].copy()
        X.accum_update()
    for i in ids:
        assert F.accum_read(i)[1] == D.accum_read(i)[1] == counts[i] + 1 and same_nan(F.accum_read(i)[0], D.accum_read(i)[0])
    D.close()
    F.close()


def test_a_period_of_one_step():
    """P = 1 in every kind, four updates with a NaN and an infinite sample: RUNMEAN is (0.0 * val + v) / 1.0, so a NaN or infinite val
    stays NaN; TIMEAVG zeroes, adds, divides by 1.0 and writes the destination on every update; RUNACCUM does not read its period."""
    n = 193
    D = st.ELMState(n)
    entries = [("t_ref2m", accum.RUNMEAN, 1, "t10"), ("t_ref2m", accum.TIMEAVG, 1, "n_melt"), ("t_ref2m", accum.RUNACCUM, 1, "micro_sigma")]
    for e in entries:
        D.accum_add(*e)
    c = np.arange(n) % 4
    rng = np.random.default_rng(93)
    val, counts = [np.zeros(n) for _ in entries], [0] * 3
    dst = {e[3]: D[e[3]] for e in entries}
    for step in range(1, 5):
        t = 280.0 + 15.0 * rng.standard_normal(n)
        if step == 2:
            t[c == 1], t[c == 2], t[c == 3] = np.nan, np.inf, -0.0
        D["t_ref2m"] = t
        D.accum_update()
        _fold_and_compare(D, entries, val, dst, {"t_ref2m": _soa(D["t_ref2m"])}, counts, step)
        assert all(accum.writes_destination(e[1], 1, step) for e in entries)
        finite = np.isfinite(t)
        assert same_nan(val[1][finite & ~np.signbit(t)], t[finite & ~np.signbit(t)]) and same_nan(D["n_melt"], val[1])  # the sample itself
        if step == 2:
            assert np.isnan(val[0][c == 1]).all() and (val[0][c == 2] == np.inf).all() and (val[1][c == 2] == np.inf).all()
            assert (val[1][c == 3] == 0.0).all() and not np.signbit(val[1][c == 3]).any()  # +0.0 + -0.0
        if step >= 3:  # 0.0 * NaN and 0.0 * inf are NaN: the running mean never recovers; the period average does
            assert np.isnan(val[0][(c == 1) | (c == 2)]).all() and np.isfinite(val[0][(c == 0) | (c == 3)]).all() and np.isfinite(val[1]).all()
    D.close()


def test_chained_entries_are_refused():
    """All rows run in one launch, so no entry may read what another writes: refused in either order of registration, with nothing
    changed and the context usable."""
    n = 193
    D = st.ELMState(n)
    f = {k: v[0] for k, v in D.fields.items()}
    a = D.accum_add("n_melt", accum.RUNMEAN, 4)
    b = D.accum_add("t_ref2m", accum.RUNMEAN, 4, "t10")
    held = D.device_bytes
    assert _invalid(D.lib.elmk_accum_add(D.ctx, f["t_ref2m"], accum.RUNMEAN, 4, f["n_melt"]))  # would write entry a's source
    assert _invalid(D.lib.elmk_accum_add(D.ctx, f["t10"], accum.TIMEAVG, 4, -1))  # would read entry b's destination
    assert D.device_bytes == held
    v = 260.0 + np.arange(n, dtype=np.float64)
    D["t_ref2m"] = v
    D["n_melt"] = v[::-1].copy()
    D.accum_update()
    for e, want in ((a, v[::-1]), (b, v)):
        got, cnt = D.accum_read(e)
        assert cnt == 1 and bits(got) == bits(accum.update(np.zeros(n), want, accum.RUNMEAN, 4, 1))
    assert D.accum_add("t_grnd", accum.TIMEAVG, 4) == 2
    D.close()


def test_update_in_a_captured_graph_advances_the_count():
    """elmk_accum_update captured once on a caller's stream and replayed: every replay is one update (the count lives on the device)."""
    n = 193
    D = st.ELMState(n)
    e = D.accum_add("t_ref2m", accum.TIMEAVG, 4, "t10")
    t = 250.0 + np.arange(n, dtype=np.float64)
    D["t_ref2m"] = t
    with captured(D) as cap:
        D.accum_update()
        cap.end()
        assert D.accum_read(e)[1] == 0  # captured, not run
        cap.replay(6)
        val = np.zeros(n)
        for k in range(1, 7):
            val = accum.update(val, t, accum.TIMEAVG, 4, k)
        got, cnt = D.accum_read(e)
        assert cnt == 6 and bits(got) == bits(val)
        assert bits(D["t10"]) == bits(t)  # the average of the one whole period
    D.close()


# ---- t10 fed back through the run --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return _inputs(200, 131)


def _host_feedback(D, rec, steps, val, n0, history=False):
    """The loop the device update replaces: after every step the host downloads t_ref2m, applies accum.update and uploads t10."""
    cons, fo, fb = [], [], []
    for s in range(len(steps)):
        c, o, b = stepwise(D, rec, steps[s:s + 1])
        val = accum.update(val, D["t_ref2m"], accum.RUNMEAN, P10, n0 + s + 1)
        D["t10"] = val
        if history:
            D.history_accumulate()
        cons.append(c[0])
        fo.append(o[0])
        fb.append(b[0])
    return (np.array(cons), np.array(fo, np.uint32), np.array(fb, np.int64)), val


def _run_context(base, graph):
    D = device(base)
    D.set_graph(graph)
    e = accum.add_t10(D, DT, period=P10)
    D.run_reserve(NREC, NSTEPS)
    upload_series(D, base[5])
    return D, e


def test_t10_feedback_through_the_run(base):
    cols, rec = base[0], base[5]
    steps = schedule()
    A = device(base)
    want, val = _host_feedback(A, rec, steps, np.zeros(200), 0)
    want_state = {k: A[k] for k in A.fields if k not in SERIES}
    A.close()
    for graph in (True, False):
        B, e = _run_context(base, graph)
        B.run(DT, steps, st.RUN_ACCUM)
        for g, w in zip(B.run_diagnostics(), want):
            assert same(g, w), graph
        for k, v in want_state.items():
            assert same(B[k], v), (graph, k)
        got, cnt = B.accum_read(e)
        assert cnt == NSTEPS and bits(got) == bits(val)
        B.close()
    # without the flag t10 stays what was uploaded, and photosynthesis sees the difference
    F, _ = _run_context(base, True)
    F.run(DT, steps)
    assert same(F["t10"], cols["t10"]) and not same(F["t10"], want_state["t10"])
    assert F.accum_read(0)[1] == 0
    assert any(not same(F[k], want_state[k]) for k in ("t_veg", "eflx_sh_veg", "qflx_tran_veg", "eflx_lh_tot"))
    F.close()


def test_seeding_from_the_destination(base):
    """accum_init without values: val = the t10 that was uploaded, the window already full; one update gives ((P-1) * t10 + v) / P."""
    cols = base[0]
    D = device(base)
    e = accum.add_t10(D, DT, period=P10)
    D.accum_init(e, None, P10 + 3)
    got, cnt = D.accum_read(e)
    assert cnt == P10 + 3 and bits(got) == bits(cols["t10"])
    v = 275.0 + 0.25 * np.arange(200)
    D["t_ref2m"] = v
    D.accum_update()
    want = (np.float64(P10 - 1) * cols["t10"] + v) / np.float64(P10)
    got, cnt = D.accum_read(e)
    assert cnt == P10 + 4 and bits(got) == bits(want) and bits(D["t10"]) == bits(want)
    # values and a count from a restart file
    D.accum_init(e, want[::-1].copy(), 2)
    D.accum_update()
    got, cnt = D.accum_read(e)
    assert cnt == 3 and bits(got) == bits(accum.update(want[::-1], v, accum.RUNMEAN, P10, 3))
    D.close()


# ---- restart -------------------------------------------------------------------------------------------------------------------------
FLAGS = st.RUN_ACCUM | st.RUN_HISTORY


def _register(D):
    """t10 fed back, a period average that is mid-period after N steps, a 20-level running mean, and a tape of t10."""
    ids = [accum.add_t10(D, DT, period=P10), D.accum_add("t_grnd", accum.TIMEAVG, 4), D.accum_add("t_soisno", accum.RUNMEAN, 10)]
    return ids, D.history_add(0, "t10", "avg")


def _sub(base, c0, n):
    cols, scal, soil, lat, lon, rec = base
    return ({k: v[c0:c0 + n] for k, v in cols.items()}, scal, soil, lat[c0:c0 + n], lon[c0:c0 + n],
            {k: v[:, c0:c0 + n] for k, v in rec.items()})


def _restart_context(base, fields=True):
    D = device(base)
    if not fields:
        for name, (fid, nlev, dt) in D.fields.items():
            D.fill(name, np.nan if dt == np.float64 else 3.0)
    D.set_graph(True)
    ids, tape = _register(D)
    D.run_reserve(NREC, NSTEPS)
    upload_series(D, base[5])
    return D, ids, tape


def _snapshot(D, ids, tape):
    out = {k: D[k] for k in D.fields if k not in SERIES}
    for i in ids:
        out[f"accum{i}"], out[f"count{i}"] = D.accum_read(i)
    out["hist"], out["samples"] = D.history_read(tape), D.history_count(0)
    return out


def _assert_same(a, b, c0=None, m=None):
    for k, v in a.items():
        w = b[k]
        if c0 is not None and isinstance(w, np.ndarray):
            w = w[..., c0:c0 + m] if k.startswith("accum") and w.ndim == 2 else w[c0:c0 + m]
        assert same(v, w) if isinstance(v, np.ndarray) else v == w, k


@pytest.fixture(scope="module")
def continuous(base):
    """2N steps that never stop, and the image after the first N."""
    A, ids, tape = _restart_context(base)
    A.run(DT, schedule()[:N], FLAGS)
    img = A.restart_save()
    A.run(DT, schedule()[N:], FLAGS)
    snap = _snapshot(A, ids, tape)
    A.close()
    return img, snap


def test_exact_restart(base, continuous):
    img, want = continuous
    p = R.verify(img)
    assert int(p["header"]["version"]) == 2 and [int(x) for x in p["accum"]["nsteps"]] == [N, N, N]
    assert [int(x) for x in p["accum"]["period"]] == [P10, 4, 10] and N % 4 != 0  # the period average is mid-period
    assert [int(s["kind"]) for s in p["sections"]].count(R.ACCUM_SECTION) == 3
    D, ids, tape = _restart_context(base, fields=False)
    D.restart_load(img)
    assert [D.accum_read(i)[1] for i in ids] == [N, N, N] and D.history_count(0) == N
    D.run(DT, schedule()[N:], FLAGS)
    _assert_same(_snapshot(D, ids, tape), want)
    D.close()


def test_restart_across_a_change_of_decomposition(base, continuous):
    img, want = continuous
    parts = []
    for c0, m in ((0, 120), (120, 80)):
        sub = _sub(base, c0, m)
        D, ids, tape = _restart_context(sub, fields=False)
        D.restart_load(R.slice(img, c0, m), c0)
        D.run(DT, schedule()[N:], FLAGS)
        _assert_same(_snapshot(D, ids, tape), want, c0, m)
        parts.append(D.restart_save(c0))
        D.close()
    full = R.verify(R.merge(parts[::-1]))
    assert [int(x) for x in full["accum"]["nsteps"]] == [2 * N] * 3 and int(full["header"]["ncols"]) == 200
    for s, d in zip(full["sections"], full["data"]):
        if int(s["kind"]) == R.ACCUM_SECTION:
            assert bits(d.reshape(want[f"accum{int(s['id'])}"].shape)) == bits(want[f"accum{int(s['id'])}"])


def test_no_entries_is_the_version_1_image(base):
    D = device(base)
    size0 = D.restart_size()
    img0 = D.restart_save()
    assert int(R.verify(img0)["header"]["version"]) == 1 and img0.size == size0
    bytes0 = D.device_bytes
    accum.add_t10(D, DT)
    assert D.restart_size() > size0 and D.device_bytes > bytes0
    D.accum_clear()
    assert D.restart_size() == size0 and D.device_bytes == bytes0
    assert bits(D.restart_save()) == bits(img0)
    D.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _invalid(rc):
    return rc == -1  # ELMK_E_INVALID


def test_refusals_change_nothing(base):
    D = device(base)
    lib, ctx, f = D.lib, D.ctx, {k: v[0] for k, v in D.fields.items()}
    nf = lib.elmk_num_fields()
    e0 = D.accum_add("t_ref2m", accum.RUNMEAN, 4, "t10")
    e1 = D.accum_add("t_grnd", accum.TIMEAVG, 4)
    D.accum_update()

    def state():
        return ([D.accum_read(e) for e in (e0, e1)], D.device_bytes, D.restart_size(), {k: D[k] for k in ("t10", "t_ref2m", "t_grnd", "n_melt", "csol")})

    def unchanged(a, b):
        return (all(x[1] == y[1] and same(x[0], y[0]) for x, y in zip(a[0], b[0])) and a[1:3] == b[1:3]
                and all(same(a[3][k], b[3][k]) for k in a[3]))

    before = state()
    add_cases = {"source -1": (-1, 0, 4, -1), "source past the end": (nf, 0, 4, -1), "kind -1": (f["t_ref2m"], -1, 4, -1),
                 "kind 3": (f["t_ref2m"], 3, 4, -1), "period 0": (f["t_ref2m"], 0, 0, -1), "period -5": (f["t_ref2m"], 0, -5, -1),
                 "destination -2": (f["t_ref2m"], 0, 4, -2), "destination past the end": (f["t_ref2m"], 0, 4, nf),
                 "destination not F64": (f["snl"], 0, 4, f["nrad"]), "destination of other levels": (f["t_ref2m"], 0, 4, f["csol"]),
                 "destination not SURFACE": (f["t_ref2m"], 0, 4, f["t_grnd"]), "destination is the source": (f["n_melt"], 0, 4, f["n_melt"]),
                 "destination taken": (f["t_grnd"], 0, 4, f["t10"])}
    for what, a in add_cases.items():
        assert _invalid(lib.elmk_accum_add(ctx, *a)), what
        assert unchanged(before, state()), what
    init_cases = {"entry -1": (-1, None, 0), "entry 2": (2, None, 0), "negative count": (e0, None, -1), "nothing to seed from": (e1, None, 0)}
    for what, a in init_cases.items():
        assert _invalid(lib.elmk_accum_init(ctx, *a)), what
        assert unchanged(before, state()), what
    buf = np.zeros(200)
    cnt = C.c_int64()
    for what, a in {"entry 2": (2, 0, 200), "columns past the end": (e0, 1, 200), "negative col0": (e0, -1, 10)}.items():
        assert _invalid(lib.elmk_accum_read(ctx, a[0], buf.ctypes.data_as(C.c_void_p), a[1], a[2], st.LAYOUT_SOA, C.byref(cnt))), what
    # a stream being captured
    with captured(D) as cap:
        rcs = [lib.elmk_accum_add(ctx, f["t_ref2m"], 0, 4, -1), lib.elmk_accum_init(ctx, e0, None, 5), lib.elmk_accum_clear(ctx)]
        cap.end()
        assert all(_invalid(rc) for rc in rcs), rcs
    assert unchanged(before, state())
    # elmk_restart_load: another accumulator table
    img = D.restart_save()
    others = []
    for table in ([("t_ref2m", accum.RUNMEAN, 5, "t10"), ("t_grnd", accum.TIMEAVG, 4, None)],  # another period
                  [("t_ref2m", accum.RUNMEAN, 4, None), ("t_grnd", accum.TIMEAVG, 4, None)],  # another destination
                  [("t_ref2m", accum.TIMEAVG, 4, "t10"), ("t_grnd", accum.TIMEAVG, 4, None)],  # another kind
                  [("t_grnd", accum.TIMEAVG, 4, None), ("t_ref2m", accum.RUNMEAN, 4, "t10")],  # another order
                  [("t_ref2m", accum.RUNMEAN, 4, "t10")], []):  # fewer entries, none (a version-1 image)
        O = st.ELMState(200)
        for e in table:
            O.accum_add(*e)
        others.append(O.restart_save())
        assert _invalid(lib.elmk_restart_load(ctx, 0, others[-1].ctypes.data, others[-1].size)), table
        assert unchanged(before, state()), table
        assert _invalid(O.lib.elmk_restart_load(O.ctx, 0, img.ctypes.data, img.size)), table
        O.close()
    assert int(R.parse(others[-1])["header"]["version"]) == 1
    damaged = img.copy()
    damaged[int(R.parse(img)["sections"][-1]["offset"]) + 9] ^= 4  # a value row of the last accumulator
    assert _invalid(lib.elmk_restart_load(ctx, 0, damaged.ctypes.data, damaged.size))
    damaged = img.copy()
    damaged[R.HEADER.itemsize + 8 + 24] ^= 1  # the step count of entry 0: covered by the header checksum
    assert _invalid(lib.elmk_restart_load(ctx, 0, damaged.ctypes.data, damaged.size))
    assert unchanged(before, state())
    # the table fills up at ELMK_ACCUM_MAX_ENTRIES; the context is still usable
    for _ in range(accum.MAX_ENTRIES - 2):
        D.accum_add("t_grnd", accum.RUNACCUM, 3)
    full = D.device_bytes
    assert _invalid(lib.elmk_accum_add(ctx, f["t_grnd"], 0, 4, -1)) and D.device_bytes == full
    want = accum.update(before[0][0][0], D["t_ref2m"], accum.RUNMEAN, 4, 2)
    D.restart_load(D.restart_save())
    D.accum_update()
    got, n = D.accum_read(e0)
    assert n == 2 and bits(got) == bits(want) and bits(D["t10"]) == bits(want)
    # ELMK_RUN_ACCUM without an entry is refused
    D.accum_clear()
    D.run_reserve(NREC, NSTEPS)
    upload_series(D, base[5])
    a = np.ascontiguousarray(schedule(), dtype=st.RUN_STEP_DTYPE)
    assert _invalid(lib.elmk_run(ctx, DT, a.ctypes.data_as(C.c_void_p), int(a.size), st.RUN_ACCUM))
    D.run(DT, schedule()[:1])
    D.sync()
    D.close()


# ---- the demo ------------------------------------------------------------------------------------------------------------------------
def test_accum_demo(tmp_path):
    """examples/accum_demo.cc builds and runs 48 steps with t10 on the device against the loop with a host round trip per step."""
    n = 320
    cols, scal, soil, lat, lon, rec = _inputs(n, 75, nrec=25)
    exe = build_demo("accum_demo", tmp_path)
    (tmp_path / "state.bin").write_bytes(state_blob(H.oracle_state(cols, scal, soil), DT, demo_records(lat, lon, rec) + [("steps", schedule(48))]))
    r = run_demo(exe, tmp_path / "state.bin")
    assert "bit-identical" in r.stdout
