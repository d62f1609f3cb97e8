"""Soil hydrology on the host (include/elmk.h "soil hydrology"; elmkernels_amd/hydrology.py): hand-checked columns of `step`, the exact
water budget of one step, the parameter helpers, the header's constants and symbols, and restart images of version 4.  The generators of
the stage's inputs are tests/hydrology_cases.py."""
import math
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests.hydrology_cases import BRANCHES, CLOSURE_BOUND, CLOSURE_MEASURED, DT, N, column, generated, host_chain
from tests.support import ROOT


# ---- hand-built columns -----------------------------------------------------------------------------------------------------------
def test_a_dry_column_stays_put():
    """Nothing falls, nothing is taken, nothing conducts (hksat = 0) and nothing drains: every store keeps its bits."""
    for zwt in (1.0, 8.0):
        c = column(zwt=zwt)
        o = hy.column(c, DT)
        assert o["liq"] == c["liq"] and o["ice0"] == 0.0 and o["h2osfc"] == 0.0 and o["wa"] == c["wa"] and o["zwt"] == zwt
        assert [o[k] for k in hy.DIAGNOSTICS] == [0.0] * 7
        assert o["vol"] == [c["liq"][j] / (c["dz"][j] * 1000.0) + 0.0 / (c["dz"][j] * 917.0) for j in range(N)]


def test_rain_on_a_saturated_column_goes_to_h2osfc():
    """Every layer full, the water table at the surface: the rain infiltrates (it is below qinmax), the solve cannot place it, and
    the excess-water pass hands it up layer by layer into h2osfc."""
    rain = 1.0e-4
    c = column(zwt=0.0, sat=1.0, hksat=0.01, qflx_top_soil=rain)
    hit = set()
    o = hy.column(c, DT, hit)
    assert {"jwt_0", "excess_up", "excess_to_h2osfc"} <= hit and "infiltration_excess" not in hit
    assert o["qflx_infl"] == rain and o["qflx_surf"] == 0.0
    assert abs(o["h2osfc"] - rain * DT) < 1.0e-9 * rain * DT + 64 * 2.0 ** -52 * max(c["liq"])
    assert all(o["liq"][j] <= 0.45 * (c["dz"][j] * 1.0e3) * (1.0 + 2.0 ** -52) for j in range(N))  # (liq[0] - xs1 rounds once)
    # and with nothing conducting, the rain never enters: infiltration excess, straight into the store
    o = hy.column(column(zwt=0.0, sat=1.0, hksat=0.0, qflx_top_soil=rain), DT)
    assert o["qflx_infl"] == 0.0 and o["h2osfc"] == rain * DT and o["liq"] == column(sat=1.0)["liq"]


def test_water_table_inside_and_below_the_column():
    """Inside (jwt < N) the bottom is sealed: the aquifer row is decoupled, drainage comes out of the layers at and below the table
    and qcharge only moves zwt.  Below (jwt == N) the aquifer is row N: wa takes the recharge and gives the drainage."""
    kw = dict(hksat=0.005, rsub_top_max=1.0e-3)
    hit = set()
    c = column(zwt=1.0, **kw)
    o = hy.column(c, DT, hit)
    assert {"jwt_mid", "drain_soil"} <= hit and "jwt_N" not in hit
    assert o["qflx_drain"] > 0.0 and o["wa"] == c["wa"]  # (the walk ends inside the column: nothing is left for the aquifer)
    tol = 64 * 2.0 ** -52 * max(max(c["liq"]), c["wa"])
    assert abs((sum(o["liq"]) - sum(c["liq"])) + o["qflx_drain"] * DT) <= tol
    assert o["zwt"] != c["zwt"]
    hit = set()
    c = column(zwt=8.0, **kw)
    o = hy.column(c, DT, hit)
    assert {"jwt_N", "drain_aquifer"} <= hit
    assert abs((o["wa"] - c["wa"]) - (o["qcharge"] - o["qflx_drain"]) * DT) <= tol
    assert abs((sum(o["liq"]) - sum(c["liq"])) + o["qcharge"] * DT) <= tol
    # the cold start sits below the column
    assert hy.cold_start_zwt(3.8019) == (3.8019 + 25.0) - 20.0 and hy._jwt(hy.cold_start_zwt(3.8019), c["zi"]) == N


def test_frozen_layers_impede():
    """qinmax = (1 - fsat) * min over the top three layers of 10^(-6 icefrac) * hksat: ice in layer 1 alone sets it."""
    rain = 0.02
    c = column(hksat=0.01, qflx_top_soil=rain)
    frac = 0.5
    c["ice"][1] = frac * 0.45 * c["dz"][1] * 917.0
    hit = set()
    o = hy.column(c, DT, hit)
    icefrac = min(1.0, min(0.45, c["ice"][1] / (c["dz"][1] * 917.0)) / 0.45)
    want = math.pow(10.0, -6.0 * icefrac) * 0.01
    assert {"imped", "infiltration_excess"} <= hit and want < 0.01 * 2.0e-3 * 1.01
    assert o["qflx_infl"] == rain - (rain - want) and o["h2osfc"] == (rain - want) * DT
    free = hy.column(column(hksat=0.01, qflx_top_soil=rain), DT)
    assert free["qflx_infl"] == rain - (rain - 0.01) and free["qflx_infl"] > 100.0 * o["qflx_infl"]


def test_the_watmin_search():
    """The bottom layer below watmin takes what the layers above can spare beyond watmin and the deficit; when none can, the rest
    comes out of the baseflow."""
    c = column()
    c["liq"][N - 1] = 0.001
    hit = set()
    o = hy.column(c, DT, hit)
    xs = 0.01 - 0.001
    assert {"watmin_search"} <= hit and "watmin_remainder" not in hit
    assert o["liq"][N - 1] == 0.001 + xs and o["liq"][N - 2] == c["liq"][N - 2] - xs and o["liq"][:N - 2] == c["liq"][:N - 2]
    assert o["qflx_drain"] == 0.0
    c = column()
    c["liq"] = [0.005] * N
    hit = set()
    o = hy.column(c, DT, hit)
    assert {"watmin_push_down", "watmin_search", "watmin_remainder"} <= hit
    assert all(abs(v - 0.01) <= 4 * 2.0 ** -52 * 0.05 for v in o["liq"]) and o["qflx_drain"] < 0.0  # (liq + (watmin - liq) rounds)
    assert abs((sum(o["liq"]) - sum(c["liq"])) + o["qflx_drain"] * DT) <= 32 * 2.0 ** -52 * 0.1


# ---- the generated columns --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    cols, rows = generated(1001, 77)
    hit = set()
    out, rows_out = hy.step(cols, rows, DT, hit)
    return cols, rows, out, rows_out, hit


def test_the_generated_columns_take_every_branch(gen):
    assert gen[4] == BRANCHES, BRANCHES - gen[4]


def test_budget_of_one_step(gen):
    """sum dliq + dice + dh2osfc + dwa = (qflx_top_soil - qflx_surf - soil and h2osfc evaporation - qflx_h2osfc_surf - sum rootsoi -
    qflx_drain + the dew and sublimation of a snow-free top layer) * dt, in every generated column.  Tolerance: the summation's
    rounding, 2^-52 times the column's largest term times the number of additions - 10 layers on either side, the three other stores,
    the ten terms of the right-hand side and the 3 * 11 products of the tridiagonal rows behind sum dliq: 64."""
    cols, rows, out, rows_out, _ = gen
    n = rows.shape[1]
    s0, s1 = hy.NLEVSNO, hy.NLEVSNO + N
    worst = 0.0
    for i in range(n):
        fh, fsno = float(cols["frac_h2osfc"][i]), float(cols["frac_sno_eff"][i])
        snl0 = int(cols["snl"][i]) == 0
        qevap = float(cols["qflx_evap_grnd"][i] if snl0 else cols["qflx_ev_soil"][i])
        top = float(cols["qflx_top_soil"][i])
        ice0, ice1 = float(cols["h2osoi_ice"][i, s0]), float(out["h2osoi_ice"][i, s0])
        terms = [top, -rows_out[hy.QFLX_SURF, i], -(1.0 - fsno - fh) * qevap, -fh * float(cols["qflx_ev_h2osfc"][i]),
                 -rows_out[hy.QFLX_H2OSFC_SURF, i], -float(cols["qflx_rootsoi"][i, :N].sum()), -rows_out[hy.QFLX_DRAIN, i]]
        if snl0:
            terms.append((1.0 - fh) * float(cols["qflx_dew_grnd"][i]))
        lhs = float((out["h2osoi_liq"][i, s0:s1] - cols["h2osoi_liq"][i, s0:s1]).sum()) + (float(out["h2osfc"][i]) - float(cols["h2osfc"][i]))
        lhs += rows_out[hy.WA, i] - rows[hy.WA, i]
        # (the ice of the top layer follows G exactly, including its clamp at zero, which is no flux of the budget)
        err = lhs - sum(terms) * DT
        big = max(rows[hy.WA, i], float(np.abs(cols["h2osoi_liq"][i, s0:s1]).max()), float(cols["h2osfc"][i]), max(abs(t) for t in terms) * DT)
        assert abs(err) <= 64 * 2.0 ** -52 * big, (i, err, big)
        worst = max(worst, abs(err) / big)
        if snl0:
            dew = (1.0 - fh) * float(cols["qflx_dew_snow"][i]) * DT
            sub = float(cols["qflx_sub_snow"][i]) * DT
            want = 0.0 if sub > ice0 + dew else (ice0 + dew) - (1.0 - fh) * float(cols["qflx_sub_snow"][i]) * DT
            assert ice1 == want
        else:
            assert ice1 == ice0
    assert worst > 0.0


def test_step_leaves_the_rest_alone(gen):
    cols, rows, out, rows_out, _ = gen
    s0, s1 = hy.NLEVSNO, hy.NLEVSNO + N
    assert set(out) == set(hy.WRITES)
    assert np.array_equal(out["h2osoi_liq"][:, :s0], cols["h2osoi_liq"][:, :s0]) and np.array_equal(out["h2osoi_liq"][:, s1:], cols["h2osoi_liq"][:, s1:])
    assert np.array_equal(out["h2osoi_ice"][:, s0 + 1:], cols["h2osoi_ice"][:, s0 + 1:])
    assert np.array_equal(out["h2osoi_vol"][:, N:], cols["h2osoi_vol"][:, N:])
    assert np.array_equal(rows_out[hy.HKSAT:hy.QFLX_SURF], rows[hy.HKSAT:hy.QFLX_SURF])
    assert np.isfinite(rows_out).all() and (rows_out[hy.ZWT] >= 0.0).all() and (rows_out[hy.ZWT] <= 80.0).all()
    assert (out["h2osoi_liq"][:, s0:s1] >= 0.01 - 1e-12).all() and (rows_out[hy.WA] <= 5000.0).all()


def test_fp32_inputs_round_once():
    """State fields are widened as stored and a result is rounded once to the stored type."""
    cols, rows = generated(40, 5)
    c32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in cols.items()}
    wide = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in c32.items()}
    o32, r32 = hy.step(c32, rows, DT)
    o64, r64 = hy.step(wide, rows, DT)
    assert r32.tobytes() == r64.tobytes()
    for k in hy.WRITES:
        assert o32[k].dtype == np.float32
    s0, s1 = hy.NLEVSNO, hy.NLEVSNO + N
    assert np.array_equal(o32["h2osoi_liq"][:, s0:s1], o64["h2osoi_liq"][:, s0:s1].astype(np.float32))
    assert np.array_equal(o32["h2osfc"], o64["h2osfc"].astype(np.float32))
    # downloads of the fp32-state build come widened: `stored` names the type they are rounded to
    ow, rw = hy.step(wide, rows, DT, stored=np.float32)
    assert rw.tobytes() == r64.tobytes() and all(ow[k].dtype == np.float64 and np.array_equal(ow[k], o32[k].astype(np.float64)) for k in hy.WRITES)


@pytest.fixture(scope="module")
def chain():
    cols, scal, soil, rows = generated(1001, 77, full=True, chain=True)
    return (cols, scal, soil, rows), host_chain(cols, scal, soil, rows), host_chain(cols, scal, soil, rows, stage=False)


def test_the_host_chain_closes_the_water_budget(chain):
    """Six steps of the oracle's physics with the stage after each: on the snow-free columns without surface water - more than half
    of all - errh2o of the closed budget stays under CLOSURE_BOUND (measured: CLOSURE_MEASURED) and its median is rounding, while
    without the stage the same quantity is of the order of (rain - evaporation) * dt."""
    _, (S, rows, with_stage), (_, _, without) = chain
    worst = 0.0
    for (e, keep), (e0, keep0) in zip(with_stage, without):
        assert keep.mean() > 0.5 and keep0.mean() > 0.5
        worst = max(worst, float(np.abs(e[keep]).max()))
        assert np.median(np.abs(e[keep])) < 1.0e-9 and np.median(np.abs(e0[keep0])) > 1.0e-3
    assert abs(worst - CLOSURE_MEASURED) < 1.0e-6 and worst < CLOSURE_BOUND
    assert np.isfinite(rows).all()


# ---- parameters, constants, symbols -----------------------------------------------------------------------------------------------
def test_parameter_helpers():
    hk = hy.hksat_from_texture(np.full((2, N), 50.0), np.full((2, N), 20.0), np.zeros((2, N)), np.linspace(0.01, 3.0, N)[None, :].repeat(2, 0))
    assert hk.shape == (N, 2) and hk[0, 0] == 0.0070556 * math.pow(10.0, -0.884 + 0.0153 * 50.0)
    peat = hy.hksat_from_texture(np.full((1, N), 50.0), np.full((1, N), 20.0), np.full((1, N), 130.0), np.full((1, N), 0.1))
    assert peat[0, 0] == max(0.28 - 0.2799 * 0.1 / 0.5, 0.0001)  # all organic, all of it connected
    t = hy.h2osfc_thresh(np.array([0.0, 0.02, 0.04]))
    assert t[0] == 0.0 and 0.0 < t[1] < t[2] and abs(t[2] / t[1] - 2.0) < 1e-12  # the depth scales with sigma
    assert hy.k_wet(np.array([0.0, 90.0]))[1] == 1.0 and hy.rsub_top_max(np.array([30.0]))[0] == 10.0 * math.sin(30.0 * (math.pi / 180.0))
    e = hy.water_balance_error(100.0, 101.0, 4000.0, 3999.5, 1e-3, 0.0, 2e-4, 0.0, 1e-4, 0.0, 5e-4, DT)
    assert e == (101.0 + 3999.5) - (100.0 + 4000.0) - (1e-3 + 0.0 - (1e-4 + 0.0 + 5e-4) - 2e-4 - 0.0) * DT


def test_header_constants_and_symbols():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    enum = dict(re.findall(r"(ELMK_HYD_[A-Z0-9_]+) = (\d+)", h))
    want = {"ZWT": hy.ZWT, "WA": hy.WA, "HKSAT": hy.HKSAT, "WTFACT": hy.WTFACT, "H2OSFC_THRESH": hy.H2OSFC_THRESH, "K_WET": hy.K_WET,
            "RSUB_TOP_MAX": hy.RSUB_TOP_MAX, "QFLX_SURF": hy.QFLX_SURF, "QFLX_INFL": hy.QFLX_INFL, "QFLX_H2OSFC_SURF": hy.QFLX_H2OSFC_SURF,
            "QFLX_DRAIN": hy.QFLX_DRAIN, "QFLX_RSUB_SAT": hy.QFLX_RSUB_SAT, "QCHARGE": hy.QCHARGE, "FSAT": hy.FSAT, "NROWS": hy.NROWS}
    assert {k: int(enum["ELMK_HYD_" + k]) for k in want} == want and st.HYD_NROWS == hy.NROWS and st.HYD_NLAYER == N
    assert re.search(r"#define ELMK_HYD_NLAYER 10\b", h) and re.search(r"#define ELMK_RUN_HYDROLOGY 32\b", h) and st.RUN_HYDROLOGY == 32
    assert re.search(r"ELMK_RESTART_HYDROLOGY = 5\b", h) and R.HYDROLOGY_SECTION == 5
    assert re.search(r"#define ELMK_RESTART_VERSION_HYDROLOGY 4u", h) and R.VERSION_HYDROLOGY == 4
    for name in ("enable", "set_params", "init", "read", "clear"):
        assert f"elmk_soil_hydrology_{name}" in L.SIGNATURES and re.search(rf"\bint elmk_soil_hydrology_{name}\(", h)
    assert "elmk_soil_hydrology" in L.SIGNATURES and re.search(r"\bint elmk_soil_hydrology\(elmk_ctx \*ctx, double dt\);", h)
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_soil_hydrology.hip")).read()
    for name, v in (("DENH2O", hy.DENH2O), ("DENICE", hy.DENICE), ("E_ICE", hy.E_ICE), ("SMPMIN", hy.SMPMIN), ("WATMIN", hy.WATMIN),
                    ("PC", hy.PC), ("MU", hy.MU), ("FFF_S", hy.FFF_S), ("FFF_D", hy.FFF_D), ("AQUIFER_MAX", hy.AQUIFER_MAX),
                    ("ROUS_MIN", hy.ROUS_MIN)):
        m = re.search(rf"HY_{name} = (-?[0-9.e+-]+)", k)
        assert m and float(m.group(1)) == v, name


# ---- restart images of version 4 ----------------------------------------------------------------------------------------------------
def _image(gcol0, n, alt, seed):
    rng = np.random.default_rng(seed)
    h = np.zeros((), R.HEADER)
    h["magic"], h["real_bytes"], h["schema_hash"], h["gcol0"], h["ncols"] = R.MAGIC, 8, 1234, gcol0, n
    kinds = [(R.FIELD, 3, 2)] + ([(R.ALT_SECTION, w, 1) for w in range(3)] if alt else []) + [(R.HYDROLOGY_SECTION, hy.ZWT, 1),
                                                                                                (R.HYDROLOGY_SECTION, hy.WA, 1)]
    sec = np.zeros(len(kinds), R.SECTION)
    data = []
    for i, (kind, ident, nlev) in enumerate(kinds):
        d = rng.standard_normal((nlev, n))
        sec[i] = (kind, ident, nlev, 0, n, 0, R.checksum(d, gcol0))
        data.append(d)
    return R.build(h, np.zeros(0, R.ENTRY), sec, data), data


@pytest.mark.parametrize("alt", [False, True], ids=["hydrology", "alt+hydrology"])
def test_restart_version_4_parse_merge_slice(alt):
    a, da = _image(0, 96, alt, 1)
    b, db = _image(96, 64, alt, 2)
    pa = R.verify(a)
    assert int(pa["header"]["version"]) == 4
    kinds = [int(k) for k in pa["sections"]["kind"]]
    assert kinds[-2:] == [R.HYDROLOGY_SECTION] * 2 and (R.ALT_SECTION in kinds) == alt
    assert [int(i) for i in pa["sections"]["id"][-2:]] == [hy.ZWT, hy.WA]
    for got, want in zip(pa["data"], da):
        assert np.array_equal(np.asarray(got).reshape(want.shape), want)
    m = R.merge([a, b])
    pm = R.verify(m)
    assert int(pm["header"]["version"]) == 4 and int(pm["header"]["ncols"]) == 160
    assert np.array_equal(np.asarray(pm["data"][-1]).reshape(1, -1), np.concatenate([da[-1], db[-1]], axis=1))
    s = R.slice(m, 96, 64)
    ps = R.verify(s)
    assert int(ps["header"]["version"]) == 4 and int(ps["header"]["gcol0"]) == 96
    for got, want in zip(ps["data"], db):
        assert np.array_equal(np.asarray(got).reshape(want.shape), want)
    # an image of another version that holds the sections, or a version-4 image without them, is refused
    bad = a.copy()
    hdr = np.frombuffer(bad[:R.HEADER.itemsize].tobytes(), R.HEADER).copy()
    hdr["version"] = 3
    bad[:R.HEADER.itemsize] = np.frombuffer(hdr.tobytes(), np.uint8)
    with pytest.raises(R.RestartError):
        R.parse(bad)
