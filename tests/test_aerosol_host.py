"""Aerosol deposition on the host: aerosol.interpolate (the numpy restatement of include/elmk.h "aerosol deposition") against a scalar
loop written straight from the spec, its edge values, the synthetic climatology, and the declarations."""
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import aerosol
from elmkernels_amd import state as st
from tests.support import ROOT, bits_f64

NEW_SYMBOLS = ("elmk_aerosol_reserve", "elmk_aerosol_upload", "elmk_aerosol_deposition", "elmk_aerosol_clear")


def bits1(x):
    return struct.pack("<d", float(x))


def scalar_remap(idx, w, a, c):
    """Column c of cell values a through the ELL map, one operation per line (Python floats are IEEE fp64)."""
    v = float(w[0][c]) * float(a[idx[0][c]])
    for k in range(1, len(idx)):
        if idx[k][c] >= 0:
            t = float(w[k][c]) * float(a[idx[k][c]])
            v = v + t
    return v


def scalar_interpolate(series, m1, m2, wt1, wt2, idx, w, ncols):
    out = {}
    for s in aerosol.STREAMS:
        a = series[s]
        col = []
        for c in range(ncols):
            r1 = float(a[m1][c]) if idx is None else scalar_remap(idx, w, a[m1], c)
            r2 = float(a[m2][c]) if idx is None else scalar_remap(idx, w, a[m2], c)
            t1 = float(wt1) * r1
            t2 = float(wt2) * r2
            col.append(t1 + t2)
        out[s] = np.array(col)
    return out


def padded_map(n, ncells, seed):
    """npts = 3 with -1 padding in rows 1 and 2 of some columns; weights that do not sum to one."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, ncells, (3, n)).astype(np.int32)
    w = rng.random((3, n)) + 0.1
    idx[1, rng.random(n) < 0.4] = -1
    idx[2, rng.random(n) < 0.5] = -1
    if n > 2:
        idx[1:, 2] = -1
    return idx, w


CASES = [(11, 0, 0.3, 0.7), (4, 4, 0.25, 0.75), (0, 1, 1.0, 0.0), (6, 7, 0.0, 1.0)]


@pytest.mark.parametrize("mapped", [False, True])
def test_interpolate_equals_the_scalar_loop(mapped):
    n, ncells = 23, 7
    series = aerosol.synthetic_climatology(ncells if mapped else n, seed=3)
    idx, w = padded_map(n, ncells, 5) if mapped else (None, None)
    if mapped:
        assert (idx[1:] < 0).any() and (idx[1:] >= 0).any()
    for m1, m2, wt1, wt2 in CASES:
        got = aerosol.interpolate(series, m1, m2, wt1, wt2, idx, w)
        want = scalar_interpolate(series, m1, m2, wt1, wt2, idx, w, n)
        assert tuple(got) == aerosol.STREAMS
        for s in aerosol.STREAMS:
            assert got[s].shape == (n,) and got[s].dtype == np.float64
            assert bits_f64(got[s]) == bits_f64(want[s]), (s, m1, m2)
    # the array form [11, 12, ncells] and the aer_ keys are the same series
    arr = np.stack([series[s] for s in aerosol.STREAMS])
    pre = {"aer_" + s: v for s, v in series.items()}
    for alt in (arr, pre):
        got = aerosol.interpolate(alt, 11, 0, 0.3, 0.7, idx, w)
        for s in aerosol.STREAMS:
            assert bits_f64(got[s]) == bits_f64(aerosol.interpolate(series, 11, 0, 0.3, 0.7, idx, w)[s])


def test_weights_one_and_zero_are_products_not_copies():
    """(1, 0) and (0, 1) evaluate x * 1 + y * 0 as written: a finite other month leaves x (up to the sign of zero), a NaN or an
    infinity in the other month propagates - NaN * 0 and inf * 0 are NaN.  A driver that wants a hole in its data ignored must
    not leave a NaN in a month of the bracket."""
    series = aerosol.synthetic_climatology(5, seed=1)
    x, y = series["bcphi"][0].copy(), series["bcphi"][1].copy()
    got = aerosol.interpolate(series, 0, 1, 1.0, 0.0)["bcphi"]
    assert np.array_equal(got, x) and bits_f64(got) == bits_f64(x * 1.0 + y * 0.0)
    got = aerosol.interpolate(series, 0, 1, 0.0, 1.0)["bcphi"]
    assert np.array_equal(got, y)
    series["bcphi"][1, 3] = np.nan
    series["bcphi"][1, 4] = np.inf
    got = aerosol.interpolate(series, 0, 1, 1.0, 0.0)["bcphi"]
    assert math.isnan(got[3]) and math.isnan(got[4]) and np.array_equal(got[:3], x[:3])
    # the other streams do not see it
    assert np.isfinite(aerosol.interpolate(series, 0, 1, 1.0, 0.0)["bcpho"]).all()


def test_bracket_december_january():
    series = aerosol.synthetic_climatology(9, seed=2)
    got = aerosol.interpolate(series, 11, 0, 0.3, 0.7)
    for s in aerosol.STREAMS:
        want = np.array([0.3 * float(series[s][11][c]) + 0.7 * float(series[s][0][c]) for c in range(9)])
        assert bits_f64(got[s]) == bits_f64(want)
    for bad in ((12, 0), (0, -1)):
        with pytest.raises(ValueError):
            aerosol.interpolate(series, bad[0], bad[1], 0.5, 0.5)
    with pytest.raises(ValueError):
        aerosol.interpolate(series, 0, 1, 0.5, 0.5, idx=np.zeros((1, 9), np.int32))


def test_negative_zero_cell_through_the_single_term_map():
    """Cell 0 of dst1_1 is -0.0 in January: with the one-term map of weight 1.0, r1 = 1.0 * -0.0 = -0.0, and the result has the bits
    of wt1 * (-0.0) + wt2 * x: +0.0 when wt2 * x is +0.0 (round to nearest: -0.0 + +0.0 = +0.0), -0.0 only when both terms are."""
    ncells = 7
    series = aerosol.synthetic_climatology(ncells, seed=4)
    assert bits1(series["dst1_1"][0, 0]) == bits1(-0.0)
    idx = np.array([[0, 0, 3]], np.int32)
    w = np.ones((1, 3))
    x = float(series["dst1_1"][1, 0])
    assert x > 0.0
    for wt1, wt2 in ((0.3, 0.7), (1.0, 0.0), (1.0, -0.0), (-1.0, 0.0)):
        got = aerosol.interpolate(series, 0, 1, wt1, wt2, idx, w)["dst1_1"]
        want = wt1 * (1.0 * -0.0) + wt2 * (1.0 * x)
        assert bits1(got[0]) == bits1(want) == bits1(got[1]), (wt1, wt2)
    assert bits1(aerosol.interpolate(series, 0, 1, 1.0, 0.0, idx, w)["dst1_1"][0]) == bits1(0.0)
    assert bits1(aerosol.interpolate(series, 0, 1, 1.0, -0.0, idx, w)["dst1_1"][0]) == bits1(-0.0)
    # same month twice: still two products and a sum
    assert bits1(aerosol.interpolate(series, 0, 0, 0.25, 0.75, idx, w)["dst1_1"][0]) == bits1(0.25 * -0.0 + 0.75 * -0.0) == bits1(-0.0)


def test_synthetic_climatology_is_seasonal_with_its_edge_cells():
    ncells = 40
    series = aerosol.synthetic_climatology(ncells, seed=6)
    assert tuple(series) == aerosol.STREAMS
    for s, a in series.items():
        assert a.shape == (12, ncells) and a.dtype == np.float64 and np.isfinite(a).all() and (a >= 0.0).all()
        assert not a[:, 1].any() and not a[:, ncells - 2].any()  # exactly zero cells
        if s.startswith("dst"):
            tot = a.sum(axis=1)
            assert int(np.argmax(tot)) == 3 and tot[3] > 5.0 * tot[9]  # April over October
    assert bits1(series["dst1_1"][0, 0]) == bits1(-0.0)
    again = aerosol.synthetic_climatology(ncells, seed=6)
    assert all(bits_f64(series[s]) == bits_f64(again[s]) for s in aerosol.STREAMS)
    m1, m2, w1, w2 = aerosol.month_bracket(0.0)
    assert (m1, m2) == (11, 0) and w1 + w2 == 1.0
    m1, m2, w1, w2 = aerosol.month_bracket(16.0)  # just past mid January
    assert (m1, m2) == (0, 1) and 0.9 < w1 < 1.0 and w1 + w2 == 1.0


# ---- declarations -----------------------------------------------------------------------------------------------------------------
def test_aerosol_abi_is_declared_and_mirrored():
    hdr = open(os.path.join(ROOT, "include", "elmk.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L.SIGNATURES
    assert re.search(r"#define ELMK_RUN_AEROSOL " + str(st.RUN_AEROSOL) + r"\b", hdr) and st.RUN_AEROSOL == aerosol.RUN_AEROSOL == 8
    assert (st.RUN_QBOT_IS_RH, st.RUN_HISTORY, st.RUN_ACCUM, st.RUN_AEROSOL) == (1, 2, 4, 8)
    # the stream order is the field order of include/elmk_fields.def, consecutive
    fields = re.findall(r"^ELMK_FIELD\((\w+),", open(os.path.join(ROOT, "include", "elmk_fields.def")).read(), re.M)
    i0 = fields.index("aer_bcphi")
    assert tuple(fields[i0:i0 + 11]) == aerosol.FIELDS == tuple("aer_" + s for s in aerosol.STREAMS)
    assert len(aerosol.STREAMS) == 11 and aerosol.NMONTHS == 12
    for m in ("aerosol_reserve", "aerosol_upload", "aerosol_deposition", "aerosol_clear"):
        assert callable(getattr(st.ELMState, m))
    import inspect

    assert inspect.signature(st.ELMInterface.run).parameters["update_aerosol"].default is False
    cpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    for name in NEW_SYMBOLS + ("ELMK_RUN_AEROSOL",):
        assert name in cpp, name


def test_library_exports_the_symbols_and_keeps_the_field_ids():
    lib = L.load()
    ids = [lib.elmk_field_id(f.encode()) for f in aerosol.FIELDS]
    assert ids == list(range(ids[0], ids[0] + 11)) and ids[0] > 0
    for f in aerosol.FIELDS:
        assert st.field_class(f) == st.CLASS_SURFACE


@pytest.mark.parametrize("src", ["examples/aerosol_demo.cc", "include/elmk_interface.hpp"])
def test_demo_and_interface_compile(src, tmp_path):
    """Syntax only: nothing is linked or run here (tests/test_gpu_aerosol.py builds and runs the demo)."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    unit = tmp_path / "unit.cc"
    unit.write_text(f'#include "{os.path.join(ROOT, src)}"\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(unit)],
                   check=True)
