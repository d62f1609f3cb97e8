"""elmkernels_amd/diagnostics.py: reduce_min_max_sum, the host restatement of the device's conservation reduction, against a literal
per-thread loop of the order include/elmk.h describes (no GPU).  tests/test_gpu_diagnostics.py holds the device to the restatement."""
import numpy as np
import pytest

from elmkernels_amd import diagnostics as dg
from tests.support import words_f64

NPART, BLOCK = 512, 256
T = NPART * BLOCK


def _min(acc, v):
    return v if (v < acc or v != v) else acc


def _max(acc, v):
    return v if (v > acc or v != v) else acc


def _tree(a):
    """One workgroup: a = list of 256 (min, max, sum) triples -> a[0] after s = 128, 64, .., 1."""
    a = list(a)
    s = len(a) // 2
    while s:
        for t in range(s):
            a[t] = (_min(a[t][0], a[t + s][0]), _max(a[t][1], a[t + s][1]), a[t][2] + a[t + s][2])
        s //= 2
    return a[0]


def literal(x):
    """Thread by thread, element by element, in Python floats (IEEE fp64): no padding, no vectorisation."""
    x = [float(v) for v in x]
    n = len(x)
    ident = (float("inf"), float("-inf"), 0.0)
    part = []
    for b in range(NPART):
        if b * BLOCK >= n:  # a workgroup none of whose threads has an element: the identity triple
            part.append(ident)
            continue
        th = []
        for t in range(BLOCK):
            mn, mx, sm = ident
            for i in range(b * BLOCK + t, n, T):
                mn, mx, sm = _min(mn, x[i]), _max(mx, x[i]), sm + x[i]
            th.append((mn, mx, sm))
        part.append(_tree(th))
    th = []
    for j in range(BLOCK):
        mn, mx, sm = ident
        for i in range(j, NPART, BLOCK):
            mn, mx, sm = _min(mn, part[i][0]), _max(mx, part[i][1]), sm + part[i][2]
        th.append((mn, mx, sm))
    return np.array(_tree(th))


def wide_values(n, seed):
    """Magnitudes log-uniform over 1e-8 .. 1e+8, random signs, some exact cancellations (x, -x pairs) and signed zeros."""
    rng = np.random.default_rng(seed)
    x = 10.0 ** rng.uniform(-8.0, 8.0, n) * rng.choice([-1.0, 1.0], n)
    k = n // 8
    if k:
        i = rng.permutation(n)[:2 * k]
        x[i[k:]] = -x[i[:k]]
    if n >= 16:
        x[rng.integers(0, n, 2)] = [0.0, -0.0]
    return x


@pytest.mark.parametrize("n", [1, 300, 131072 + 7])
def test_restatement_equals_the_literal_thread_loop(n):
    x = wide_values(n, 100 + n % 97)
    got, want = dg.reduce_min_max_sum(x), literal(x)
    assert np.array_equal(words_f64(got), words_f64(want)), (n, got, want)
    assert got[0] == x.min() and got[1] == x.max()
    if n > 1:  # the order is visible in these values: numpy's pairwise sum and the running sum round differently
        assert words_f64(got[2]) != words_f64(np.sum(x)) and words_f64(got[2]) != words_f64(np.cumsum(x)[-1])


@pytest.mark.parametrize("n,at,what", [(300, a, w) for a in (0, 137, 299) for w in (np.nan, np.inf, -np.inf)]
                         + [(131072 + 7, 131072 + 3, np.nan)])  # (the last: a column only the second trip reaches)
def test_non_finite_values(n, at, what):
    """A NaN anywhere makes min, max and sum NaN; an infinity is an ordinary value; +inf with -inf sums to NaN."""
    x = wide_values(n, 7)
    x[at] = what
    got, want = dg.reduce_min_max_sum(x), literal(x)
    assert np.array_equal(got, want, equal_nan=True)
    if np.isnan(what):
        assert np.isnan(got).all()
    else:
        assert got[0] == x.min() and got[1] == x.max() and got[2] == what
        x[(at + n // 2) % n] = -what
        got = dg.reduce_min_max_sum(x)
        assert got[0] == -np.inf and got[1] == np.inf and np.isnan(got[2])
        assert np.array_equal(got, literal(x), equal_nan=True)


def test_padding_with_plus_zero_changes_no_bit():
    """The vectorised form adds +0.0 where a device thread adds nothing.  s + (+0.0) has the bits of s for every s but -0.0, and an
    accumulator that starts at +0.0 never becomes -0.0: (+0.0) + (-0.0) = +0.0, x + (-x) = +0.0, and a sum of terms none of which is
    -0.0 is not -0.0 either.  So a column of nothing but -0.0 (the only candidate) still sums to +0.0 on both paths."""
    s = np.array([1.5, -1.5, 1e-320, -1e-320, 1e308, -1e308, np.inf, -np.inf, 0.0, 4.9e-324])
    assert np.array_equal(words_f64(s + 0.0), words_f64(s))
    assert words_f64(np.float64(-0.0) + np.float64(0.0)) == words_f64(0.0) and words_f64(np.float64(0.0) + np.float64(-0.0)) == words_f64(0.0)
    assert words_f64(np.float64(2.5) + np.float64(-2.5)) == words_f64(0.0)
    for n in (1, 2, 300):
        x = np.full(n, -0.0)
        got = dg.reduce_min_max_sum(x)
        assert words_f64(got[2]) == words_f64(0.0) and np.array_equal(words_f64(got), words_f64(literal(x)))
    x = wide_values(300, 5)
    x[:5] = -0.0
    assert np.array_equal(words_f64(dg.reduce_min_max_sum(x)), words_f64(literal(x)))


def test_empty_and_identity():
    """No columns: the identities (what an all-identity stage 2 gives)."""
    got = dg.reduce_min_max_sum(np.zeros(0))
    assert got[0] == np.inf and got[1] == -np.inf and words_f64(got[2]) == words_f64(0.0)
