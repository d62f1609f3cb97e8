"""Per-column solar geometry on the host (no GPU): elmk_sin of elmkernels_amd/csrc/elmk_math.h against the live libm, and the
host build of elmkernels_amd/csrc/elmk_solar.h (the precompute of elmk_set_column_geography / elmk_solar_geometry, then the
per-column routine k_solar.hip runs) against include/elmk_interface.hpp's elmk::solar and, where oracle/_ref is built, against
the reference's own incident_shortwave.cc / day_length.cc - bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.support import ROOT

CSRC = os.path.join(ROOT, "elmkernels_amd", "csrc")


def _gcc():
    if shutil.which("gcc") is None or shutil.which("g++") is None:
        pytest.skip("no gcc")


@pytest.fixture(scope="module")
def sin_checker(tmp_path_factory):
    _gcc()
    exe = str(tmp_path_factory.mktemp("sinchk") / "sin_host_check")
    # -ffp-contract=off: only the explicit fma() calls of the header may be fused; -mfma: they are one instruction
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp", os.path.join(ROOT, "tests", "tools", "sin_host_check.c"),
                           "-o", exe, "-lm"])
    return exe


@pytest.fixture(scope="module")
def solar_libs(tmp_path_factory):
    _gcc()
    d = tmp_path_factory.mktemp("solar")
    mine, shim = str(d / "columns.so"), str(d / "shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(ROOT, "tests", "c", "solar_columns.cc"), "-o", mine])
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "solar_shim.cc"), "-o", shim])
    a, b = C.CDLL(mine), C.CDLL(shim)
    a.elmk_test_solar_columns.argtypes = [C.c_long] + [C.c_void_p] * 9
    a.elmk_test_solar_columns.restype = None
    a.elmk_test_solar_geography_ok.argtypes = [C.c_double, C.c_double]
    a.elmk_test_solar_geography_ok.restype = C.c_int
    b.elmk_test_solar.argtypes = [C.c_int64] + [C.c_void_p] * 7
    b.elmk_test_solar.restype = None
    return a, b


def test_host_build_of_device_sin_matches_libm_bit_for_bit(sin_checker):
    """5 argument classes x 4 M arguments (|x| <= 3 pi; |x| <= 2e8, compared below 105414350; random bit patterns below
    105414350; tiny values and subnormals; the range boundaries of s_sin.c, multiples of pi/2, specials): zero mismatches."""
    r = subprocess.run([sin_checker, "4000000", "20261015"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "mismatches=" in ln]
    assert len(lines) == 5 and all(ln.endswith("mismatches=0") for ln in lines), r.stdout
    compared = sum(int(ln.split("n=")[1].split()[0]) for ln in lines)
    assert compared >= 20_000_000 - 4_000_000, r.stdout  # (class 1 compares about half of its arguments)


def solar_cases(n, seed):
    """(lat, lon, dt, decday, doy): random over the globe and the year, plus the edges - the poles (and the 10 eps beyond
    them that day_length.cc accepts), the equator, the dateline, midnight, the solstices and equinoxes, polar day and night."""
    rng = np.random.default_rng(seed)
    lat = np.arcsin(2.0 * rng.random(n) - 1.0)
    lon = (rng.random(n) - 0.5) * 2.0 * np.pi
    dt = rng.choice([60.0, 1800.0, 3600.0, 10800.0, 86400.0], n)
    decday = 1.0 + 365.0 * rng.random(n)
    k = n // 20
    eps10 = 10.0 * np.finfo(float).eps
    lat[:k] = rng.choice([np.pi / 2, -np.pi / 2, np.pi / 2 + eps10, -(np.pi / 2 + eps10), 0.0, -0.0, 1.4, -1.4], k)  # poles, equator, polar
    lon[k:2 * k] = rng.choice([np.pi, -np.pi, 0.0, 3.0 * np.pi / 2], k)  # dateline, Greenwich, beyond +pi
    decday[2 * k:3 * k] = np.floor(decday[2 * k:3 * k])  # midnight: the fractional day is exactly zero
    decday[3 * k:4 * k] = rng.choice([80.0, 172.0, 173.5, 266.0, 355.0, 356.25, 1.0, 365.99], k)  # equinoxes, solstices, year ends
    lat[3 * k:4 * k] = rng.choice([1.45, -1.45, 1.2, -1.2], k)  # polar day and polar night at the solstices
    doy = decday.astype(np.int32) - 1  # date.doy with decday = decimal_doy(date) + 1 (init_timestep_kokkos.cc:29)
    return lat, lon, dt, decday, doy


def run_columns(lib, lat, lon, dt, decday, doy):
    n = lat.size
    out = [np.zeros(n) for _ in range(4)]
    doy = np.ascontiguousarray(doy, dtype=np.int32)
    lib.elmk_test_solar_columns(n, lat.ctypes.data, lon.ctypes.data, dt.ctypes.data, decday.ctypes.data, doy.ctypes.data,
                                *[o.ctypes.data for o in out])
    return out  # cosz, dayl, max_dayl, dayl_factor


def run_pointwise(fn, lat, lon, dt, decday):
    n = lat.size
    out = [np.zeros(n) for _ in range(3)]
    fn(n, lat.ctypes.data, lon.ctypes.data, dt.ctypes.data, decday.ctypes.data, *[o.ctypes.data for o in out])
    return out  # average_cosz, daylength of declination_angle_sin((int)decday), max_daylength


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def test_column_routine_matches_elmk_solar_and_the_reference(solar_libs):
    """elmk_solar.h's split (time-invariant column terms and per-step scalars on the host, the rest per column with elmk_sin /
    elmk_acos) gives average_cosz, daylength and max_daylength with the bits of elmk::solar (include/elmk_interface.hpp) on
    10^6 tuples, and - where oracle/_ref is built - of the reference's own sources; the day-length factor is canopy_fluxes'."""
    mine_lib, shim = solar_libs
    lat, lon, dt, decday, doy = solar_cases(1_000_000, 20261015)
    cosz, dayl, max_dayl, dfac = run_columns(mine_lib, lat, lon, dt, decday, doy)
    want = run_pointwise(shim.elmk_test_solar, lat, lon, dt, decday)
    for a, b, what in zip((cosz, dayl, max_dayl), want, ("average_cosz", "daylength", "max_daylength")):
        assert same_bits(a, b), (what, int(np.sum(a.view(np.uint64) != b.view(np.uint64))))
    assert (cosz > 0).mean() > 0.3 and (cosz == 0).mean() > 0.2  # day and night both sampled
    assert (cosz[3 * 50_000:4 * 50_000] == 0).any() and (cosz[3 * 50_000:4 * 50_000] > 0).any()
    assert len(np.unique(max_dayl)) >= 2  # both hemispheres
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (dayl * dayl) / (max_dayl * max_dayl)
    q = np.where(0.01 < q, q, 0.01)  # std::max(0.01, q): NaN (0 / 0: max_dayl is 0 south of the equator) gives 0.01
    assert same_bits(dfac, np.where(q < 1.0, q, 1.0))

    from oracle import oracle as O

    if not O.have_ref() or not hasattr(O.Reference().R, "elmref_solar"):
        pytest.skip("oracle/_ref/libelmref.so not built here")
    R = O.Reference().R
    R.elmref_solar.argtypes = [C.c_int64] + [C.c_void_p] * 7
    R.elmref_solar.restype = None
    ref = run_pointwise(R.elmref_solar, lat, lon, dt, decday)
    for a, b, what in zip((cosz, dayl, max_dayl), ref, ("average_cosz", "daylength", "max_daylength")):
        assert same_bits(a, b), what


def test_geography_range_is_the_references():
    """elmk_set_column_geography accepts what day_length.cc:22 asserts (|lat| <= pi/2 + 10 eps) and finite longitudes only."""
    _gcc()
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "c.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", "c", "solar_columns.cc"),
                               "-o", so])
        ok = C.CDLL(so).elmk_test_solar_geography_ok
        ok.argtypes = [C.c_double, C.c_double]
        eps10 = 10.0 * np.finfo(float).eps
        assert ok(np.pi / 2 + eps10, 0.0) and ok(-np.pi / 2 - eps10, 3.0) and ok(0.0, -7.0)
        assert not ok(np.nextafter(np.pi / 2 + eps10, 4.0), 0.0) and not ok(-2.0, 0.0)
        assert not ok(np.nan, 0.0) and not ok(0.0, np.nan) and not ok(0.0, np.inf)
