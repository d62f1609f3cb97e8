"""Per-column solar geometry on the device (elmk_set_column_geography / elmk_solar_geometry, k_solar.hip) and per-column day
length in canopy_fluxes: against the reference's own incident_shortwave.cc / day_length.cc (oracle/_ref), against the oracle run
group by group with each group's (dayl, max_dayl) as the scalars, and against scalar-mode device runs."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.run_cases import DT, _device_step, _global_pair, _groups, _oracle_step
from tests.support import ROOT, build_demo, run_demo

pytestmark = pytest.mark.gpu



def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _ref_solar():
    from oracle import oracle as O

    if not O.have_ref() or not hasattr(O.Reference().R, "elmref_solar"):
        pytest.skip("oracle/_ref/libelmref.so not built (build() makes it where the reference is mounted)")
    R = O.Reference().R
    R.elmref_solar.argtypes = [C.c_int64] + [C.c_void_p] * 7
    R.elmref_solar.restype = None
    return R.elmref_solar


def _pointwise(fn, lat, lon, dt, decday):
    n = lat.size
    full = [np.ascontiguousarray(np.broadcast_to(v, (n,)), dtype=np.float64) for v in (lat, lon, dt, decday)]
    out = [np.zeros(n) for _ in range(3)]
    fn(n, *[a.ctypes.data for a in full], *[o.ctypes.data for o in out])
    return out


def _shim(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path / "shim.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "solar_shim.cc"), "-o", so])
    f = C.CDLL(so).elmk_test_solar
    f.argtypes = [C.c_int64] + [C.c_void_p] * 7
    f.restype = None
    return f


def test_device_sin_matches_libm():
    """math_eval("sin"): the host libm's bits on more than 10^6 arguments - the physics range, |x| <= 2e8 (below 105414350), random bit
    patterns, tiny and subnormal values, specials."""
    rng = np.random.default_rng(5)
    k = 250_000
    bits = rng.integers(0, 0x419921FB00000000, k, dtype=np.uint64).view(np.float64)
    wide = (rng.random(k) - 0.5) * 4e8
    wide = wide[np.abs(wide) < 105414350.0]
    x = np.concatenate([(rng.random(k) - 0.5) * 6 * np.pi, wide, bits, -bits,
                        rng.integers(0, 0x3EB0000000000000, k, dtype=np.uint64).view(np.float64),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, np.pi, -np.pi / 2])])
    D = st.ELMState(64)
    got = D.math_eval("sin", x)
    D.close()
    libm = C.CDLL("libm.so.6")  # the host libm itself (numpy's sin may be its own vectorised routine)
    libm.sin.restype = C.c_double
    libm.sin.argtypes = [C.c_double]
    want = np.fromiter((libm.sin(v) for v in x.tolist()), dtype=np.float64, count=x.size)
    ok = (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))
    assert x.size >= 1_000_000 and ok.all(), x[~ok][:5]


def test_solar_geometry_matches_the_reference_over_the_globe(tmp_path):
    """elmk_solar_geometry at 262 144 columns over the globe for several steps (midnight, a solstice, a day step, the first
    and last day of the year): coszen, dayl and max_dayl bit-identical to the reference's own sources (oracle/_ref) and to
    elmk::solar; day and night both present."""
    ref, shim = _ref_solar(), _shim(tmp_path)
    n = 262_144
    lat, lon = synth.global_grid(n, seed=21)
    D = st.ELMState(n)
    D.set_column_geography(lat, lon)
    for dt, decday in ((1800.0, 172.0), (1800.0, 172.4375), (3600.0, 80.75), (86400.0, 300.0), (1800.0, 1.0), (1800.0, 365.98)):
        D.solar_geometry(dt, decday, int(decday) - 1)
        cosz = D["coszen"].reshape(-1)
        dayl, max_dayl = D.day_length()
        for fn in (ref, shim):
            want = _pointwise(fn, lat, lon, dt, decday)
            for a, b, what in zip((cosz, dayl, max_dayl), want, ("coszen", "dayl", "max_dayl")):
                assert same_bits(a, b), (what, dt, decday, int((a.view(np.uint64) != b.view(np.uint64)).sum()))
        if dt < 86400.0:
            assert (cosz > 0).any() and (cosz == 0).any()
    D.close()


@pytest.mark.parametrize("how,graph,half", [("per_wrapper", False, False), ("fused", False, True), ("advance", True, False),
                                            ("advance", False, True)])
def test_per_column_physics_matches_the_oracle_group_by_group(how, graph, half):
    """Per-column mode, tier B, 32 768 columns over both hemispheres: solar -> get_forcing -> phenology -> init_timestep ->
    the ten physics calls (per wrapper, fused, elmk_advance_physics plain or as a graph, the half-workgroup option) for two steps.
    Checked against the oracle run once per group of columns sharing (dayl, max_dayl), with those as its scalars: bit for bit."""
    n = 32_768
    D, cols, scal, soil = _global_pair(n, 31)
    D.set_graph(graph)
    D.set_option(st.OPT_CF_HALF_WORKGROUPS, int(half))
    oracles = {}
    for step, decday in enumerate((172.25, 172.3125)):
        D.solar_geometry(DT, decday, int(decday) - 1)
        coszen = D["coszen"].copy()
        dayl, max_dayl = D.day_length()
        groups = _groups(dayl, max_dayl)
        assert len(groups) >= 2  # the hemispheres differ (max_daylength, day_length.cc:39)
        _device_step(D, how)
        for dl, mdl, m in groups:
            key = (dl.tobytes(), mdl.tobytes())
            if key not in oracles:
                assert step == 0
                oracles[key] = H.oracle_state(cols, dict(scal, dayl=float(dl), max_dayl=float(mdl)), soil)
            _oracle_step(oracles[key], coszen)
            worst, bad = H.compare_states(D, oracles[key], skip_cols=~m, bitwise=True)
            assert not bad, (how, step, float(dl), float(mdl), bad)
    D.close()


def test_per_column_mode_equals_scalar_mode_per_group_at_262144_columns():
    """At 262 144 columns: per-column mode against a scalar-mode device run of the same state for each (dayl, max_dayl) group,
    compared on that group's columns, after a fused step (graph) and an elmk_advance_physics step."""
    n = 262_144
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=41)
    lat, lon = synth.global_grid(n, seed=41)
    D = H.device_state(cols, scal, soil)
    D.set_column_geography(lat, lon)
    D.set_graph(True)
    D.solar_geometry(DT, 100.5, 99)
    coszen = D["coszen"].copy()
    dayl, max_dayl = D.day_length()
    for f in (st.timestep7_fused, st.advance_physics):
        f(D, DT)
    names = [k for k in D.fields if k not in ("err_flags",)]
    got = {k: D[k] for k in names}
    for dl, mdl, m in _groups(dayl, max_dayl):
        B = H.device_state(cols, dict(scal, dayl=float(dl), max_dayl=float(mdl)), soil)
        B["coszen"] = coszen
        B.set_graph(True)
        for f in (st.timestep7_fused, st.advance_physics):
            f(B, DT)
        for k in names:
            a, b = got[k][m], B[k][m]
            ok = np.array_equal(a, b) if a.dtype.kind != "f" else bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
            assert ok, (k, float(dl), float(mdl))
        B.close()
    D.close()


def test_mode_rules():
    """A geography alone changes nothing; after clear the scalar baseline is back; a graph captured in scalar mode does not
    replay stale kernels in per-column mode; missing geography, NaN and |lat| > pi/2 + 10 eps are refused."""
    n = 8192
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=51)
    lat, lon = synth.global_grid(n, seed=51)

    def run(D):
        D.set_graph(True)
        st.timestep7_fused(D, DT)
        return {k: D[k] for k in ("t_veg", "btran", "eflx_sh_veg", "qflx_tran_veg", "psnsun", "psnsha") if k in D.fields}

    base = H.device_state(cols, scal, soil)
    want = run(base)
    base.close()
    D = H.device_state(cols, scal, soil)
    with pytest.raises(L.ElmkError):
        D.solar_geometry(DT, 10.5, 9)  # no geography
    bad = lat.copy()
    bad[17] = np.nan
    with pytest.raises(L.ElmkError):
        D.set_column_geography(bad, lon)
    bad[17] = np.nextafter(np.pi / 2 + 10 * np.finfo(float).eps, 4.0)
    with pytest.raises(L.ElmkError):
        D.set_column_geography(bad, lon)
    D.set_column_geography(lat, lon)
    got = run(D)  # geography alone: the scalar bits
    assert all(same_bits(got[k], want[k]) for k in want)
    # reset, switch to per-column mode with a graph already captured in scalar mode; on every group of columns the result must be
    # the one a scalar-mode context with the group's scalars gives.  South of the equator max_daylength is 0 (day_length.cc:28,39),
    # so the day-length factor there is 0.01 instead of the baseline's: a stale scalar-mode graph would not give those bits.
    for k, v in cols.items():
        D[k] = v
    D.solar_geometry(DT, 172.25, 171)
    dayl, max_dayl = D.day_length()
    coszen = D["coszen"].copy()
    got = run(D)
    groups = _groups(dayl, max_dayl)
    assert len(groups) == 2
    for dl, mdl, m in groups:
        B = H.device_state(cols, dict(scal, dayl=float(dl), max_dayl=float(mdl)), soil)
        B["coszen"] = coszen
        ref = run(B)
        B.close()
        assert all(same_bits(got[k][m], ref[k][m]) for k in got), (float(dl), float(mdl))
    south = max_dayl == 0.0
    assert south.any() and not all(same_bits(got[k][south], want[k][south]) for k in got)
    # clear: back to the scalar baseline
    D.clear_column_geography()
    for k, v in cols.items():
        D[k] = v
    got = run(D)
    assert all(same_bits(got[k], want[k]) for k in want)
    with pytest.raises(L.ElmkError):
        D.day_length()
    D.close()


def test_twelve_step_chain_with_advancing_date():
    """12 steps at 20 000 columns, decday advancing by dt / 86400 per step from late evening across midnight: the per-column
    chain (solar, phenology, forcing, init_timestep, elmk_advance_physics as a graph) stays bit-identical to the grouped oracle
    chain."""
    n = 20_000
    D, cols, scal, soil = _global_pair(n, 61)
    D.set_graph(True)
    oracles = {}
    decday0 = 200.75
    for step in range(12):
        decday = decday0 + step * DT / 86400.0
        D.solar_geometry(DT, decday, int(decday) - 1)
        coszen = D["coszen"].copy()
        dayl, max_dayl = D.day_length()
        _device_step(D, "advance")
        for dl, mdl, m in _groups(dayl, max_dayl):
            key = (dl.tobytes(), mdl.tobytes())
            if key not in oracles:
                assert step == 0
                oracles[key] = H.oracle_state(cols, dict(scal, dayl=float(dl), max_dayl=float(mdl)), soil)
            _oracle_step(oracles[key], coszen)
            worst, bad = H.compare_states(D, oracles[key], skip_cols=~m, bitwise=True)
            assert not bad, (step, bad)
    D.close()


def test_global_grid_demo_runs(tmp_path):
    """examples/global_grid_demo.cc compiles against include/ and libelmk and steps a simulated day over both hemispheres."""
    r = run_demo(build_demo("global_grid_demo", tmp_path), "4096", timeout=300)
    fr = [float(ln.split("day fraction")[1].split()[0]) for ln in r.stdout.splitlines() if "day fraction" in ln]
    assert len(fr) == 48 and min(fr) > 0.0 and max(fr) < 1.0, r.stdout
