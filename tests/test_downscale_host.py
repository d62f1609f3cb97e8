"""elmkernels_amd/downscale.py, the host restatement of the downscaling contract (include/elmk.h "downscaling"): hand-checked scalar
cases, the dz = 0 identity, the W == 0 and A == 0 branches of the longwave renormalisation and the group-map checks.  No GPU."""
import math

import numpy as np
import pytest

from elmkernels_amd import downscale as DSC
from elmkernels_amd import regrid as RG


def qsat_magnus(T, p):
    """A stand-in saturation specific humidity (Magnus form); the contract takes any qsat, the device uses the reference's."""
    T = np.asarray(T, dtype=np.float64)
    es = 611.2 * np.array([math.exp(17.62 * (t - 273.15) / (t - 30.03)) for t in T.reshape(-1)]).reshape(T.shape)
    return 0.622 * es / (np.asarray(p, dtype=np.float64) - 0.378 * es)


def one(tg, pg, qg, lg, prec, hc, hf, **kw):
    out = DSC.downscale(np.array([tg]), np.array([pg]), np.array([qg]), np.array([lg]), np.array([prec]), np.array([hc]),
                        np.array([hf]), qsat_magnus, **kw)
    return {k: float(v[0]) for k, v in out.items()}


def test_constants_are_elm_constants():
    assert DSC.RAIR == pytest.approx(287.0423, rel=1e-6)
    assert (DSC.LAPSE, DSC.LAPSE_LW, DSC.LW_LIMIT, DSC.ZBOT) == (0.006, 0.032, 0.5, 30.0)


def test_mountain_column_by_hand():
    """1 500 m above the forcing's surface: 9 K colder, about 17 % lower pressure, RH kept, longwave 48 W/m2 lower, all snow."""
    o = one(280.0, 90000.0, 0.005, 300.0, 1.0e-3, 1500.0, 0.0)
    assert o["forc_tbot"] == pytest.approx(271.0, abs=1e-12)
    hbot = DSC.RAIR * 0.5 * (280.0 + 271.0) / DSC.GRAV
    assert hbot == pytest.approx(8064.4, rel=1e-4)
    assert o["forc_pbot"] == pytest.approx(90000.0 * math.exp(-1500.0 / hbot), rel=1e-14)
    assert 0.82 < o["forc_pbot"] / 90000.0 < 0.84
    assert o["forc_thbot"] == pytest.approx(280.0 - 9.0 * math.exp(30.0 / hbot * DSC.RAIR / DSC.CPAIR), rel=1e-14)
    rh_g = 0.005 / qsat_magnus(280.0, 90000.0)
    rh_c = o["forc_qbot"] / qsat_magnus(271.0, o["forc_pbot"])
    assert rh_c == pytest.approx(rh_g, rel=1e-14)
    assert o["forc_lwrad"] == pytest.approx(300.0 - 48.0, abs=1e-12)
    assert o["forc_rain"] == 0.0 and o["forc_snow"] == 1.0e-3


def test_valley_column_and_the_rain_snow_split():
    """Below the forcing's surface it is warmer and the pressure higher; the split follows the downscaled temperature."""
    o = one(272.15, 95000.0, 0.003, 280.0, 2.0e-3, 0.0, 1000.0 / 6.0)  # dz = -166.67 m: tc = 273.15, all snow
    assert o["forc_tbot"] == pytest.approx(273.15, abs=1e-12)
    assert o["forc_pbot"] > 95000.0
    assert o["forc_rain"] == pytest.approx(0.0, abs=1e-15) and o["forc_snow"] == pytest.approx(2.0e-3, abs=1e-15)
    o = one(273.15, 95000.0, 0.003, 280.0, 2.0e-3, 0.0, 1000.0 / 6.0)  # tc = 274.15: half rain
    assert o["forc_tbot"] == pytest.approx(274.15, abs=1e-12)
    assert o["forc_rain"] == pytest.approx(1.0e-3, rel=1e-12) and o["forc_snow"] == pytest.approx(1.0e-3, rel=1e-12)
    o = one(273.15, 95000.0, 0.003, 280.0, -1.0, 0.0, 0.0)  # ProcessPREC clamps a negative record
    assert o["forc_rain"] == 0.0 and o["forc_snow"] == 0.0


def test_longwave_band():
    """Lc stays within lw_limit of Lg: clamped at both ends, untouched inside."""
    assert one(280.0, 90000.0, 0.005, 300.0, 0.0, 10000.0, 0.0)["forc_lwrad"] == 150.0
    assert one(280.0, 90000.0, 0.005, 300.0, 0.0, -10000.0, 0.0)["forc_lwrad"] == 450.0
    assert one(280.0, 90000.0, 0.005, 300.0, 0.0, 1000.0, 0.0, lw_limit=0.1)["forc_lwrad"] == 300.0 * (1.0 - 0.1)
    assert one(280.0, 90000.0, 0.005, 300.0, 0.0, 1000.0, 0.0, lapse_lw=0.0)["forc_lwrad"] == 300.0


def test_equal_heights_are_the_identity():
    """dz = 0 gives back every input bit for bit (exp(-0.0) = 1, qs / qs = 1), and the split of OFF."""
    rng = np.random.default_rng(3)
    n = 2000
    tg = 240.0 + 80.0 * rng.random(n)
    pg = 5.0e4 + 5.0e4 * rng.random(n)
    qg = 1e-4 + 0.02 * rng.random(n)
    lg = 150.0 + 300.0 * rng.random(n)
    prec = np.where(rng.random(n) < 0.3, 0.0, 1e-3 * rng.random(n))
    h = 4000.0 * rng.random(n)
    o = DSC.downscale(tg, pg, qg, lg, prec, h, h.copy(), qsat_magnus, 0.0065, 0.04, 0.3)
    for k, v in (("forc_tbot", tg), ("forc_thbot", tg), ("forc_pbot", pg), ("forc_qbot", qg), ("forc_lwrad", lg)):
        assert o[k].tobytes() == v.tobytes(), k
    frac = np.minimum(1.0, np.maximum(0.0, (tg - DSC.TFRZ) * 0.5))
    assert o["forc_rain"].tobytes() == (frac * prec).tobytes() and o["forc_snow"].tobytes() == ((1.0 - frac) * prec).tobytes()
    ptr, col, w = RG.owner_map(np.arange(n) // 150, 0.5 + rng.random(n), (n + 149) // 150)
    assert (DSC.group_norm(lg, o["forc_lwrad"], ptr, col, w) == 1.0).all()
    assert DSC.renormalise_longwave(lg, o["forc_lwrad"], ptr, col, w).tobytes() == lg.tobytes()


def test_renormalisation_keeps_the_group_mean():
    rng = np.random.default_rng(4)
    n = 1000
    lg = 200.0 + 200.0 * rng.random(n)
    lc = lg - 0.032 * rng.uniform(-1500.0, 1500.0, n)
    cell = np.arange(n) // 100
    cell[950:] = -1
    ptr, col, w = RG.owner_map(cell, 0.5 + rng.random(n), 10)
    out = DSC.renormalise_longwave(lg, lc, ptr, col, w)
    ones = np.ones(n)
    W = RG.apply_aggregate(ptr, col, w, ones, 0.0)
    assert np.allclose(RG.apply_aggregate(ptr, col, w, out, 0.0) / W, RG.apply_aggregate(ptr, col, w, lg, 0.0) / W, rtol=1e-13, atol=0)
    assert out[950:].tobytes() == lc[950:].tobytes()  # columns of no group
    # a group of one column gives back its Lg (to rounding)
    one_ptr, one_col, one_w = np.array([0, 1]), np.array([7], np.int32), np.array([0.3])
    got = DSC.renormalise_longwave(lg, lc, one_ptr, one_col, one_w)[7]
    assert abs(got - lg[7]) <= 4 * np.spacing(lg[7])


def test_zero_weight_and_zero_longwave_branches():
    """W == 0 (every weight 0, or no terms) and A == 0 (Lg 0 over the group) give norm 1: Lc as it is."""
    lg = np.array([300.0, 310.0, 0.0, 0.0, 280.0])
    lc = np.array([250.0, 260.0, 10.0, 20.0, 270.0])
    ptr = np.array([0, 2, 4, 4, 5])  # group 2 has no terms
    col = np.array([0, 1, 2, 3, 4], np.int32)
    w = np.array([0.0, 0.0, 0.5, 0.5, 1.0])
    norm = DSC.group_norm(lg, lc, ptr, col, w)
    assert norm[0] == 1.0 and norm[1] == 1.0 and norm[2] == 1.0
    assert norm[3] == (280.0 / 1.0) / (270.0 / 1.0)
    out = DSC.renormalise_longwave(lg, lc, ptr, col, w)
    assert out[:4].tobytes() == lc[:4].tobytes() and out[4] == 270.0 * norm[3]


@pytest.mark.parametrize("case", ["duplicate", "twice_in_one", "negative", "nan", "inf", "col_high", "col_low", "ptr0", "decreasing",
                                  "length", "empty"])
def test_group_map_checks(case):
    ptr, col, w = np.array([0, 2, 3]), np.array([0, 1, 2]), np.array([0.5, 0.5, 1.0])
    if case == "duplicate":
        col = np.array([0, 1, 1])
    elif case == "twice_in_one":
        col = np.array([0, 0, 2])
    elif case == "negative":
        w = np.array([0.5, -0.5, 1.0])
    elif case == "nan":
        w = np.array([0.5, np.nan, 1.0])
    elif case == "inf":
        w = np.array([0.5, 0.5, np.inf])
    elif case == "col_high":
        col = np.array([0, 1, 5])
    elif case == "col_low":
        col = np.array([-1, 1, 2])
    elif case == "ptr0":
        ptr = np.array([1, 2, 3])
    elif case == "decreasing":
        ptr = np.array([0, 3, 2])
    elif case == "length":
        ptr = np.array([0, 2, 4])
    else:
        ptr = np.array([0])
    with pytest.raises(ValueError):
        DSC.check_groups(ptr, col, w, 5)
    DSC.check_groups(np.array([0, 2, 3]), np.array([0, 1, 2]), np.array([0.5, 0.5, 0.0]), 5)  # zero weights are allowed


def test_exp_is_the_libm_per_element():
    x = np.linspace(-0.5, 0.5, 101)
    assert DSC._exp(x).tobytes() == np.array([math.exp(v) for v in x]).tobytes()
