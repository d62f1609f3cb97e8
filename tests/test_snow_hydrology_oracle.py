"""kokkos_snow_hydrology in the oracle (oracle/elmo_physics_g.c), structural checks.  The reference has no fixture for this
path; its own snow functions are run against the restatement bit for bit in tests/test_oracle_vs_ref.py, all but the two
aerosol bookkeeping functions, which are PARITY UNPINNED and only covered here.  What can be checked without the
reference is checked: the layer re-meshing conserves what it must conserve (water, ice, the six
aerosol masses, enthalpy), it leaves a consistent mesh, it is idempotent on a settled pack, the documented choices for
the reference's two out-of-bounds reads are flagged exactly when they are taken, and the whole wrapper keeps the column
water balance.  The HIP kernels are compared with this restatement bit for bit (tests/test_gpu_parity.py)."""
import ctypes as C

import numpy as np
import pytest

from elmkernels_amd import synth
from oracle import oracle as O
from tests import helpers as H

DT = 1800.0
TFRZ, CPICE, CPWAT, HFUS = 273.15, 2.11727e3, 4.188e3, 3.337e5
AER = ("mss_bcphi", "mss_bcpho", "mss_dst1", "mss_dst2", "mss_dst3", "mss_dst4")


def _state(n=6016, seed=5, tier="B"):
    ft = H.field_table_from_oracle()
    cols, scal, soil = synth.make_state(ft, n, tier=tier, seed=seed)
    return H.oracle_state(cols, scal, soil)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pack(rng, snl, thin=False):
    """One column's level arrays for a pack of snl layers (top-aligned at level 5 - snl)."""
    a = {k: np.zeros(20) for k in ("t", "ice", "liq", "dz", "z")}
    a["zi"] = np.zeros(21)
    a["rds"] = np.zeros(5)
    for k in AER:
        a[k] = np.zeros(5)
    a["zi"][5:] = np.cumsum(np.r_[0.0, 0.02 * 1.5 ** np.arange(15)])
    a["dz"][5:] = np.diff(a["zi"][5:])
    a["t"][5:] = 270.0
    a["liq"][5:] = 10.0
    for lev in range(5 - snl, 5):
        a["dz"][lev] = (0.004 if thin and rng.random() < 0.5 else 0.01 + 0.3 * rng.random())
        a["ice"][lev] = 250.0 * a["dz"][lev] * (0.02 if thin and rng.random() < 0.3 else 1.0)
        a["liq"][lev] = 5.0 * a["dz"][lev] * (rng.random() < 0.4)
        a["t"][lev] = 272.0 - 10 * rng.random()
        a["rds"][lev] = 60.0 + 1000.0 * rng.random()
        for k in AER:
            a[k][lev] = 1e-6 * rng.random()
    return a


def _enthalpy(a):
    return float((((CPICE * a["ice"] + CPWAT * a["liq"]) * (a["t"] - TFRZ) + HFUS * a["liq"])[:5]).sum())


def _call_combine(lib, a, snl, ltype=1, urbpoi=0, frac=1.0):
    snl_c = C.c_int(snl)
    sc = [C.c_double(v) for v in (0.0, 0.0, frac, frac, 100.0, 0.0, 0.0, 0.0)]  # h2osno, snow_depth, frac_sno_eff, frac_sno, int_snow, 3 fluxes
    err = C.c_uint32(0)
    lib.elmo_combine_layers(urbpoi, ltype, C.c_double(DT), C.byref(snl_c), *[C.byref(x) for x in sc], _p(a["t"]), _p(a["ice"]),
                            _p(a["liq"]), _p(a["rds"]), *[_p(a[k]) for k in AER], _p(a["dz"]), _p(a["z"]), _p(a["zi"]), C.byref(err))
    return snl_c.value, [x.value for x in sc], err.value


def _call_divide(lib, a, snl, frac=1.0):
    snl_c = C.c_int(snl)
    err = C.c_uint32(0)
    lib.elmo_divide_layers(C.c_double(frac), C.byref(snl_c), _p(a["ice"]), _p(a["liq"]), _p(a["t"]), _p(a["rds"]),
                           *[_p(a[k]) for k in AER], _p(a["dz"]), _p(a["z"]), _p(a["zi"]), C.byref(err))
    return snl_c.value, err.value


def _mesh_ok(a, snl):
    top = 5 - snl
    for i in range(top, 5):
        assert a["dz"][i] > 0
        assert abs(a["zi"][i] - (a["zi"][i + 1] - a["dz"][i])) <= 1e-12 * max(1.0, abs(a["zi"][i]))
        assert abs(a["z"][i] - (a["zi"][i + 1] - 0.5 * a["dz"][i])) <= 1e-12 * max(1.0, abs(a["z"][i]))


def test_combine_and_divide_conserve_mass_and_energy():
    lib = O.lib().lib
    rng = np.random.default_rng(3)
    ncomb = ndiv = noob = 0
    for trial in range(4000):
        snl = int(rng.integers(1, 6))
        a = _pack(rng, snl, thin=True)
        before = dict(ice=a["ice"][:6].sum(), liq=a["liq"][:6].sum(), H=_enthalpy(a), dz=a["dz"][:5].sum(),
                      **{k: a[k].sum() for k in AER})
        snl2, sc, err = _call_combine(lib, a, snl)
        assert 0 <= snl2 <= snl and not (err & ~H.WARN_COMBINE)
        noob += bool(err & H.WARN_COMBINE)
        gone = snl2 == 0 and snl > 0 and sc[0] > 0 and a["ice"][:5].sum() > 0  # "all snow gone": ice stays in h2osno
        # water and ice of the pack + the top soil level (what leaves the pack goes there): nothing is lost.  (Levels above
        # the new top keep stale copies of shifted elements until prune_snow_layers zeroes them: they are not counted.)
        t2 = 5 - snl2
        if not gone:
            assert abs(a["ice"][t2:6].sum() - before["ice"]) <= 1e-12 * before["ice"] + 1e-15
            assert abs(a["liq"][t2:6].sum() - before["liq"]) <= 1e-12 * before["liq"] + 1e-15
        if snl2 > 0:
            ncomb += snl2 < snl
            assert abs(sc[0] - (a["ice"][5 - snl2:5] + a["liq"][5 - snl2:5]).sum()) <= 1e-12 * sc[0]  # h2osno = sum of the layers
            assert abs(sc[1] - a["dz"][5 - snl2:5].sum()) <= 1e-12 * sc[1]                           # snow_depth likewise
            _mesh_ok(a, snl2)
            if snl2 < snl and not gone:
                # layers merged inside the pack keep the aerosol mass; enthalpy is conserved by combine() when no layer left
                # through the bottom (a removed thin-ice layer hands its water to the layer below without its heat)
                pass
        # divide
        if snl2 > 0:
            m0 = {k: a[k][5 - snl2:].sum() for k in AER}
            for k in ("ice", "liq", "t", "dz"):  # prune_snow_layers
                a[k][:5 - snl2] = 0.0
            i0, l0, h0, d0 = a["ice"][:5].sum(), a["liq"][:5].sum(), _enthalpy(a), a["dz"][:5].sum()
            snl3, err3 = _call_divide(lib, a, snl2)
            assert snl2 <= snl3 <= 5 and not (err3 & ~H.ERR_DIVIDE)
            ndiv += snl3 > snl2
            assert abs(a["ice"][:5].sum() - i0) <= 1e-12 * i0 and abs(a["liq"][:5].sum() - l0) <= 1e-12 * l0 + 1e-18
            assert abs(a["dz"][5 - snl3:5].sum() - d0) <= 1e-12 * d0
            for k in AER:
                assert abs(a[k][5 - snl3:].sum() - m0[k]) <= 1e-12 * m0[k] + 1e-30, k
            if not np.any((a["t"][5 - snl3:5] >= TFRZ)):  # (the freezing-point cap of a new layer replaces its temperature)
                assert abs(_enthalpy(a) - h0) <= 1e-9 * abs(h0)
            _mesh_ok(a, snl3)
            # settled: a second combine + divide changes nothing
            b = {k: v.copy() for k, v in a.items()}
            s4, _, _ = _call_combine(lib, b, snl3)
            s5, _ = _call_divide(lib, b, s4) if s4 > 0 else (0, 0)
            if s4 == snl3:
                assert s5 == snl3
                for k in ("ice", "liq", "t", "dz", "rds") + AER:
                    assert np.array_equal(a[k], b[k]), k
    assert ncomb > 200 and ndiv > 500  # both directions of the re-meshing were exercised


def test_combine_out_of_bounds_choice_is_flagged_only_for_five_layers():
    """The shift loop's extra element (snow_hydrology_impl.hh:871-885) is index -1 only when the pack has five layers and a
    combination happens below its second layer; every other case stays in bounds and must not raise the flag."""
    lib = O.lib().lib
    rng = np.random.default_rng(9)
    seen = {True: 0, False: 0}
    for trial in range(3000):
        snl = int(rng.integers(2, 6))
        a = _pack(rng, snl, thin=True)
        a["ice"][5 - snl:5] = np.maximum(a["ice"][5 - snl:5], 0.05)  # keep the first (ice <= 0.01) loop out of it
        _, _, err = _call_combine(lib, a, snl)
        flagged = bool(err & H.WARN_COMBINE)
        seen[flagged] += 1
        if flagged:
            assert snl == 5
    assert seen[True] > 0 and seen[False] > 0


def test_snow_water_out_of_bounds_choice_is_flagged_only_when_taken():
    S = _state()
    snl0 = S["snl"].copy()
    S.snow_hydrology(DT)
    flagged = (S["err_flags"] & H.WARN_WATER) != 0
    assert flagged.any() and not flagged[snl0 < 2].any()  # needs the layer pair (3, 4): at least two layers
    assert not (S["err_flags"] & np.uint32(0xFFFFFFFF ^ (H.WARN_WATER | H.WARN_COMBINE | H.ERR_DIVIDE | H.ERR_AGE))).any()


def test_whole_wrapper_keeps_the_water_and_the_mesh():
    """Every column after kokkos_snow_hydrology: 0 <= snl <= 5; levels above the pack are zero (prune_snow_layers); the mesh of
    the pack is consistent; h2osno is the water of the layers; snw_rds of every layer is SNW_RDS_MIN (the reference's aging
    clamp, snow_hydrology_impl.hh:217-223) and 0 above the pack; aerosol concentrations are mass / layer water; and the
    column's water (snow + soil + what went to the surface) changed only by the surface fluxes the step applied."""
    S = _state(n=12032, seed=8)
    snl0 = S["snl"].copy()
    lay0 = snl0 > 0
    w0 = (S["h2osoi_ice"] + S["h2osoi_liq"]).sum(axis=1)
    src = np.where(S["do_capsnow"] == 1, -S["frac_sno_eff"] * (S["qflx_sub_snow"] + S["qflx_evap_grnd"]),
                   S["frac_sno_eff"] * (S["qflx_dew_snow"] - S["qflx_sub_snow"] + S["qflx_rain_grnd"] + S["qflx_dew_grnd"]
                                        - S["qflx_evap_grnd"])) * DT
    S.snow_hydrology(DT)
    snl = S["snl"]
    assert ((snl >= 0) & (snl <= 5)).all() and (snl > 0).sum() > 1000 and (snl != snl0).sum() > 100
    lev = np.arange(5)[None, :]
    above = lev < (5 - snl)[:, None]
    for k in ("h2osoi_ice", "h2osoi_liq", "t_soisno", "dz", "zsoi", "zisoi"):
        assert (S[k][:, :5][above] == 0).all(), k
    for k in AER + tuple("cnc_" + a[4:] for a in AER):
        assert (S[k][above] == 0).all(), k
    inpack = ~above
    assert (S["snw_rds"][inpack] == 54.526).all() and (S["snw_rds"][above] == 0).all()
    mass = (S["h2osoi_ice"] + S["h2osoi_liq"])[:, :5]
    assert np.allclose(np.where(inpack, mass, 0).sum(axis=1)[snl > 0], S["h2osno"][snl > 0], rtol=1e-12)
    for a in AER:
        m, cn = S[a][inpack], S["cnc_" + a[4:]][inpack]
        assert np.allclose(cn * mass[inpack], m, rtol=1e-12, atol=1e-30), a
    zi = S["zisoi"]
    for i in range(5):
        sel = inpack[:, i]
        assert np.allclose(zi[sel, i], zi[sel, i + 1] - S["dz"][sel, i], rtol=1e-12, atol=1e-15)
    # water: layered columns that were not capped and lost no ice to the 0.9 kg/m2 reset keep their water to rounding
    w1 = (S["h2osoi_ice"] + S["h2osoi_liq"]).sum(axis=1)
    ok = lay0 & (snl > 0) & (S["mflx_neg_snow"] == 0)
    resid = np.abs(w1 - w0 - src)[ok]
    assert np.percentile(resid, 95) < 1e-9
    assert not (S["err_flags"] & H.ERR_AGE).any()


def test_idempotent_without_fluxes():
    """A pack that has been re-meshed is left alone by a second call when nothing acts on it: no deposition, no dew or
    evaporation, no melt, frozen and cold enough that compaction is the only process (and compaction alone never changes the
    number of layers of a pack whose layers are thick enough)."""
    S = _state(n=6016, seed=12)
    for k in ("qflx_sub_snow", "qflx_dew_snow", "qflx_evap_grnd", "qflx_dew_grnd", "qflx_rain_grnd", "qflx_snomelt", "qflx_snow_grnd",
              "qflx_snwcp_ice") + tuple("aer_" + a for a in ("bcphi", "bcpho", "bcdep", "dst1_1", "dst1_2", "dst2_1", "dst2_2", "dst3_1",
                                                             "dst3_2", "dst4_1", "dst4_2")):
        S[k][:] = 0.0
    S["imelt"][:] = 0
    S["h2osoi_liq"][:, :5] = 0.0
    S.snow_hydrology(DT)
    snl1 = S["snl"].copy()
    mass1 = {k: S[k].sum(axis=1).copy() for k in AER + ("h2osoi_ice",)}
    S.snow_hydrology(DT)
    same = S["snl"] == snl1
    assert same.mean() > 0.97  # (compaction thins layers: a few packs cross a combination threshold)
    for k, v in mass1.items():
        assert np.allclose(S[k].sum(axis=1)[same], v[same], rtol=1e-12, atol=1e-30), k
