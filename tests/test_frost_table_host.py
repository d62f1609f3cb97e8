"""The frost table and the perched water table on the host (include/elmk.h "soil hydrology", F'; elmkernels_amd/hydrology.py): hand-checked
columns, one per branch; the generated columns take every branch; the two bit-equality consequences of the header; the water budget of
one step with the perched drainage; the closure of a six-step chain; fp32 inputs; the parameter helper, the constants and the symbols."""
import math
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import state as st
from tests.hydrology_cases import (BRANCHES, CHAIN_STEPS, CLOSURE_BOUND, CLOSURE_FIELDS, COLD, DT, FROST_BRANCHES, S0, S1, WARM, Count, N, column,
                                   generated_frost, water_mass)
from tests.support import ROOT, bits


# ---- hand-built columns -----------------------------------------------------------------------------------------------------------
def frost_column(kf, q_perch_max=1.0e-6, **kw):
    """hydrology_cases.column with layers 0 .. kf-1 thawed and kf .. 9 frozen (kf = N: all thawed)."""
    return column(t=[WARM] * kf + [COLD] * (N - kf), q_perch_max=q_perch_max, **kw)


def run(c):
    hit = set()
    return hy.column(c, DT, hit), hit


def plain(c):
    """The same column without the extension."""
    return hy.column({k: v for k, v in c.items() if k not in ("t", "q_perch_max")}, DT)


def test_branch_a_drains_the_water_table_above_the_frost_table():
    """The water table lies in layer 5 and the frost table is the node of layer 7.  D and E are those of the column without the
    extension, which with rsub_top_max = 0 returns liq and zwt as E leaves them (F.3 to F.8 do nothing in this column); from there qp is
    the closed form, it comes out of layer jwt alone, and the water table drops inside that layer."""
    kf, hksat, qpm = 7, 0.005, 1.0e-6
    c = frost_column(kf, qpm, zwt=0.3, hksat=hksat, rsub_top_max=1.0e-3)
    o, hit = run(c)
    assert hit & (FROST_BRANCHES | {"drain_soil", "drain_aquifer"}) == {"frost_A"}
    base = hy.column(column(zwt=0.3, hksat=hksat), DT)
    zwt_e, liq_e = base["zwt"], base["liq"]
    jwt = hy._jwt(zwt_e, c["zi"])
    assert jwt == 5 and base["qflx_drain"] == 0.0
    ft = c["z"][kf]
    dzmm = [d * 1.0e3 for d in c["dz"]]
    qs, ws = 0.0, 0.0
    for j in range(jwt, kf + 1):  # no ice: imped = 10^-0 = 1
        qs = qs + 1.0 * hksat * dzmm[j]
        ws = ws + dzmm[j]
    qp = qpm * (qs / ws) * (ft - zwt_e)
    assert 0.0 < qp * DT < liq_e[jwt] - 0.01  # layer jwt holds it: rt ends at 0 and qp keeps its value
    assert o["frost_table"] == ft and o["zwt_perched"] == ft and o["qflx_drain_perched"] == qp + 0.0 / DT
    assert o["liq"][jwt] == liq_e[jwt] + (-qp * DT) and o["liq"][:jwt] == liq_e[:jwt] and o["liq"][jwt + 1:] == liq_e[jwt + 1:]
    assert o["zwt"] == zwt_e - (-qp * DT) / 0.45 / 1000.0 and zwt_e < o["zwt"] < c["zi"][jwt + 1]
    assert o["qflx_drain"] == 0.0 and o["wa"] == c["wa"]  # rsub_top = 0 and F.2 is skipped


def test_branch_a_exhausts_the_layers():
    """liq near watmin in layers jwt .. kf and a rate that asks for millimetres: every layer gives what it has above watmin, the water
    table ends at the bottom of layer kf, and qp is reduced by rt / dt, so that it is what was taken."""
    kf, qpm, hksat = 6, 1.0, 0.005
    c = frost_column(kf, qpm, zwt=0.2, hksat=hksat)
    for j in range(4, kf + 1):  # jwt = 4: zi[3] = 0.1655 < 0.2 <= zi[4] = 0.2891
        c["liq"][j] = 0.01 + 2.0 ** -10 * (j + 1)
    base = plain(c)
    o, hit = run(c)
    assert hit & FROST_BRANCHES == {"frost_A", "frost_A_exhausted"}
    zwt_e = base["zwt"]
    jwt = hy._jwt(zwt_e, c["zi"])
    assert jwt <= kf and o["zwt"] == c["zi"][kf + 1]
    qp0 = qpm * hksat * (c["z"][kf] - zwt_e)  # uniform hksat, no ice: qs = hksat up to the rounding of the mean
    taken = sum(base["liq"]) - sum(o["liq"])
    assert 0.0 < taken < 0.5 * qp0 * DT and abs(taken - o["qflx_drain_perched"] * DT) <= 64 * 2.0 ** -52 * max(c["liq"])
    assert all(abs(o["liq"][j] - 0.01) <= 4 * 2.0 ** -52 for j in range(jwt, kf + 1))
    assert o["liq"][kf + 1:] == base["liq"][kf + 1:] and o["qflx_drain"] == 0.0


def test_branch_b_perched_table_between_two_nodes():
    """The water table is deep, layers 5 and 6 are near saturation over the frost table at the node of layer 6, and layer 4 is at 0.5:
    the perched table is where the interpolation between the nodes of layers 4 and 5 reaches 0.9.  With hksat = 0 the solve moves
    nothing, so the values of F' follow from the column as given, and nothing drains; with hksat the drainage comes out of layers 5
    and 6 and everything else is the column without the extension."""
    kf, qpm = 6, 1.0e-6
    c = frost_column(kf, qpm, zwt=8.0, hksat=0.0)
    dzmm = [d * 1.0e3 for d in c["dz"]]
    for j in (5, 6):
        c["liq"][j] = 0.98 * (0.45 * dzmm[j])
    o, hit = run(c)
    assert hit & FROST_BRANCHES == {"frost_B_perched", "perched_ends_in_layer"} and "drain_aquifer" in hit
    v = [c["liq"][j] / (c["dz"][j] * 1000.0) + 0.0 / (c["dz"][j] * 917.0) for j in range(N)]
    s1, s2 = v[4] / 0.45, v[5] / 0.45
    assert s1 <= 0.9 < s2
    m = (c["z"][5] - c["z"][4]) / (s2 - s1)
    b = c["z"][5] - m * s2
    zwp = m * 0.9 + b
    assert c["z"][4] < zwp < c["z"][5]
    assert o["frost_table"] == c["z"][kf] and o["zwt_perched"] == zwp and o["qflx_drain_perched"] == 0.0 and o["liq"] == c["liq"]
    c2 = dict(c, hksat=[0.005] * N)
    o2, hit2 = run(c2)
    base = plain(c2)
    assert hit2 & FROST_BRANCHES == {"frost_B_perched", "perched_ends_in_layer"}
    assert c2["z"][3] < o2["zwt_perched"] < c2["z"][kf] and o2["qflx_drain_perched"] > 0.0
    tol = 64 * 2.0 ** -52 * max(max(c2["liq"]), c2["wa"])
    assert abs((sum(base["liq"]) - sum(o2["liq"])) - o2["qflx_drain_perched"] * DT) <= tol
    assert o2["liq"][:5] == base["liq"][:5] and o2["liq"][7:] == base["liq"][7:] and o2["liq"][5] < base["liq"][5]
    assert o2["zwt"] == base["zwt"] and o2["wa"] == base["wa"] and o2["qflx_drain"] == base["qflx_drain"]


def test_branch_b_nothing_saturated():
    """Everything at 0.5 down to the frost layer: kp == kf, nothing drains, the perched table is the frost table, and the A to H outputs
    are those of the column without the extension."""
    c = frost_column(5, zwt=8.0, hksat=0.005, rsub_top_max=1.0e-3)
    o, hit = run(c)
    assert "frost_B_none" in hit and not hit & (FROST_BRANCHES - {"frost_B_none"})
    assert o["qflx_drain_perched"] == 0.0 and o["zwt_perched"] == o["frost_table"] == c["z"][5]
    base = plain(c)
    assert {k: o[k] for k in base} == base


def test_a_thawed_column():
    c = frost_column(N, zwt=1.0, hksat=0.005, rsub_top_max=1.0e-3, sat=0.99)
    o, hit = run(c)
    assert "frost_B_thawed" in hit and not hit & (FROST_BRANCHES - {"frost_B_thawed"}) and "drain_soil" in hit
    assert o["frost_table"] == c["z"][N - 1] == o["zwt_perched"] and o["qflx_drain_perched"] == 0.0
    base = plain(c)
    assert {k: o[k] for k in base} == base


def test_a_frozen_top_layer():
    """t[0] <= tfrz and no thawed layer over a frozen one: kf = 0.  With zwt >= z[0] branch B with kp == kf == 0; with zwt above the
    node of layer 0, branch A over layer 0 alone.  A thawed layer between frozen ones moves the frost table under it."""
    c = column(t=[COLD] * N, q_perch_max=1.0e-6, zwt=1.0, hksat=0.005, rsub_top_max=1.0e-3)
    o, hit = run(c)
    assert "frost_B_none" in hit and o["frost_table"] == c["z"][0] and o["qflx_drain_perched"] == 0.0
    base = plain(c)
    assert {k: o[k] for k in base} == base
    c = column(t=[COLD] * N, q_perch_max=1.0e-6, zwt=0.001, hksat=0.0, sat=0.9)  # (nothing conducts: E leaves zwt alone)
    o, hit = run(c)
    assert "frost_A" in hit and o["frost_table"] == c["z"][0] and o["qflx_drain"] == 0.0
    c = column(t=[COLD, WARM, WARM] + [COLD] * (N - 3), q_perch_max=1.0e-6, zwt=8.0)
    o, hit = run(c)
    assert o["frost_table"] == c["z"][3]
    # a NaN water table lands in B
    c = frost_column(4, zwt=float("nan"))
    o, hit = run(c)
    assert "frost_A" not in hit and o["zwt"] != o["zwt"]


# ---- the generated columns --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gen():
    cols, rows, frost = generated_frost(1001, 77)
    hit = Count()
    out, rows_out, frost_out = hy.step(cols, rows, DT, hit, frost=frost)
    return cols, rows, frost, out, rows_out, frost_out, hit


def test_the_generated_columns_take_every_branch(gen):
    hit = gen[6]
    print({k: hit.get(k, 0) for k in sorted(FROST_BRANCHES)})
    for k in FROST_BRANCHES:
        assert hit.get(k, 0) >= 20, (k, hit.get(k, 0))
    assert BRANCHES - {"drain_aquifer", "drain_soil"} <= set(hit), BRANCHES - set(hit)
    frost_out = gen[5]
    assert np.isfinite(frost_out).all() and bits(frost_out[hy.Q_PERCH_MAX]) == bits(gen[2][hy.Q_PERCH_MAX])


def _same_outputs(a, b, sel):
    (out_a, rows_a), (out_b, rows_b) = a, b
    assert bits(rows_a[:, sel]) == bits(rows_b[:, sel])
    for k in hy.WRITES:
        assert bits(out_a[k][sel]) == bits(out_b[k][sel]), k


def test_thawed_columns_have_the_bits_of_the_plain_stage(gen):
    cols, rows, frost, out, rows_out, frost_out, _ = gen
    thawed = (cols["t_soisno"][:, S0:S1] > hy.TFRZ).all(axis=1)
    assert thawed.sum() >= 20
    plain = hy.step(cols, rows, DT)
    _same_outputs((out, rows_out), plain, thawed)
    assert bits(frost_out[hy.QFLX_DRAIN_PERCHED][thawed]) == bits(np.zeros(thawed.sum()))
    assert bits(frost_out[hy.FROST_TABLE][thawed]) == bits(cols["zsoi"][thawed, S1 - 1].astype(np.float64))
    assert bits(frost_out[hy.ZWT_PERCHED][thawed]) == bits(frost_out[hy.FROST_TABLE][thawed])


def test_without_a_rate_branch_b_has_the_bits_of_the_plain_stage(gen):
    cols, rows, frost, _, _, _, _ = gen
    zero = frost.copy()
    zero[hy.Q_PERCH_MAX] = 0.0
    n = rows.shape[1]
    in_b = np.zeros(n, bool)
    for i in range(n):
        hit = set()
        hy.step({k: np.asarray(v)[i:i + 1] for k, v in cols.items()}, rows[:, i:i + 1], DT, hit, frost=zero[:, i:i + 1])
        in_b[i] = "frost_A" not in hit
    assert 20 <= in_b.sum() <= n - 20
    out, rows_out, frost_out = hy.step(cols, rows, DT, frost=zero)
    _same_outputs((out, rows_out), hy.step(cols, rows, DT), in_b)
    assert (frost_out[hy.QFLX_DRAIN_PERCHED][in_b] == 0.0).all()


def test_budget_of_one_step(gen):
    """test_hydrology_host.test_budget_of_one_step with - qflx_drain_perched * dt among the flux terms, in the same tolerance (64
    roundings of the column's largest term); without the term the residual is qflx_drain_perched * dt to that tolerance in every
    column that drained."""
    cols, rows, frost, out, rows_out, frost_out, _ = gen
    n = rows.shape[1]
    drained = 0
    for i in range(n):
        fh, fsno = float(cols["frac_h2osfc"][i]), float(cols["frac_sno_eff"][i])
        snl0 = int(cols["snl"][i]) == 0
        qevap = float(cols["qflx_evap_grnd"][i] if snl0 else cols["qflx_ev_soil"][i])
        top = float(cols["qflx_top_soil"][i])
        qp = float(frost_out[hy.QFLX_DRAIN_PERCHED, i])
        terms = [top, -rows_out[hy.QFLX_SURF, i], -(1.0 - fsno - fh) * qevap, -fh * float(cols["qflx_ev_h2osfc"][i]),
                 -rows_out[hy.QFLX_H2OSFC_SURF, i], -float(cols["qflx_rootsoi"][i, :N].sum()), -rows_out[hy.QFLX_DRAIN, i]]
        if snl0:
            terms.append((1.0 - fh) * float(cols["qflx_dew_grnd"][i]))
        lhs = float((out["h2osoi_liq"][i, S0:S1] - cols["h2osoi_liq"][i, S0:S1]).sum()) + (float(out["h2osfc"][i]) - float(cols["h2osfc"][i]))
        lhs += rows_out[hy.WA, i] - rows[hy.WA, i]
        big = max(rows[hy.WA, i], float(np.abs(cols["h2osoi_liq"][i, S0:S1]).max()), float(cols["h2osfc"][i]), max(abs(t) for t in terms) * DT,
                  abs(qp) * DT)
        tol = 64 * 2.0 ** -52 * big
        err = lhs - sum(terms + [-qp]) * DT
        assert abs(err) <= tol, (i, err, big)
        if qp != 0.0:
            drained += 1
            without = lhs - sum(terms) * DT
            assert abs(without + qp * DT) <= tol, (i, without, qp * DT)
    assert drained >= 100


def test_fp32_inputs_round_once():
    cols, rows, frost = generated_frost(40, 5)
    c32 = {k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in cols.items()}
    wide = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in c32.items()}
    o32, r32, f32 = hy.step(c32, rows, DT, frost=frost)
    o64, r64, f64 = hy.step(wide, rows, DT, frost=frost)
    assert bits(r32) == bits(r64) and bits(f32) == bits(f64)
    assert bits(f64[hy.FROST_TABLE]) != bits(hy.step(cols, rows, DT, frost=frost)[2][hy.FROST_TABLE])  # (zsoi as stored: fp32)
    for k in hy.WRITES:
        assert o32[k].dtype == np.float32
    assert np.array_equal(o32["h2osoi_liq"][:, S0:S1], o64["h2osoi_liq"][:, S0:S1].astype(np.float32))
    ow, rw, fw = hy.step(wide, rows, DT, stored=np.float32, frost=frost)
    assert bits(rw) == bits(r64) and bits(fw) == bits(f64)
    assert all(ow[k].dtype == np.float64 and np.array_equal(ow[k], o32[k].astype(np.float64)) for k in hy.WRITES)


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def frost_closure(f, wa_beg, h2osno_beg, rows_out, dt, qp):
    """hydrology_cases.closure with the perched drainage in the source/sink (qp None: without it)."""
    e = hy.water_balance_error(f["dtbegin_column_h2o"], water_mass(f), wa_beg, rows_out[hy.WA], f["forc_rain"], f["forc_snow"],
                               f["qflx_evap_tot"], f["qflx_snwcp_ice"], rows_out[hy.QFLX_SURF], rows_out[hy.QFLX_H2OSFC_SURF],
                               rows_out[hy.QFLX_DRAIN], dt, qflx_drain_perched=qp)
    keep = (f["snl"] == 0) & (f["h2osno"] == 0.0) & (h2osno_beg == 0.0) & (f["frac_h2osfc"] == 0.0)
    return e, keep


def frost_host_chain(cols, scal, soil, rows, frost, nsteps=CHAIN_STEPS, dt=DT):
    """hydrology_cases.host_chain with the extension (frost None: without): per step (errh2o, keep, frost rows)."""
    from tests import helpers as H

    S = H.oracle_state(cols, scal, soil)
    rows = rows.copy()
    per_step = []
    for _ in range(nsteps):
        S.init_timestep()
        h2osno_beg = np.array(S.fields["h2osno"])
        S.timestep7(dt)
        S.soil_temperature(dt)
        S.snow_hydrology(dt)
        S.surface_fluxes(dt)
        wa_beg = rows[hy.WA].copy()
        if frost is None:
            out, rows = hy.step(S.fields, rows, dt)
        else:
            out, rows, frost = hy.step(S.fields, rows, dt, frost=frost)
        for k, v in out.items():
            S.fields[k][...] = v
        per_step.append(frost_closure({k: np.array(S.fields[k]) for k in CLOSURE_FIELDS}, wa_beg, h2osno_beg, rows, dt,
                                      None if frost is None else frost[hy.QFLX_DRAIN_PERCHED]) + (frost,))
    return S, rows, per_step


@pytest.fixture(scope="module")
def chain():
    cols, scal, soil, rows, frost = generated_frost(1001, 77, full=True, chain=True)
    return frost_host_chain(cols, scal, soil, rows, frost)[2], frost_host_chain(cols, scal, soil, rows, None)[2]


def test_the_host_chain_closes_the_water_budget(chain):
    """Six steps of the oracle's physics with the F' stage after each, on the snow-free columns without surface water: the maximum of
    |errh2o| with the perched drainage in the source/sink stays inside test_hydrology_host's bound (ten times the 0.9 mm literal-ice
    artefact); the median is not more than ten times the median of the same chain without the extension on the same columns (both sum
    the same number of rounded terms)."""
    with_frost, without = chain
    drained = 0
    for s, ((e, keep, frost), (e0, keep0, _)) in enumerate(zip(with_frost, without)):
        both = keep & keep0
        assert both.mean() > 0.5
        med, med0, worst = float(np.median(np.abs(e[both]))), float(np.median(np.abs(e0[both]))), float(np.abs(e[keep]).max())
        print(f"step {s}: kept {both.mean():.3f}, max |errh2o| {worst:.17g}, median with the extension {med:.3e}, without {med0:.3e}")
        assert worst < CLOSURE_BOUND
        assert med <= 10.0 * med0
        drained += int((frost[hy.QFLX_DRAIN_PERCHED][both] != 0.0).sum())
    assert drained >= 100


# ---- the parameter, constants, symbols --------------------------------------------------------------------------------------------
def test_q_perch_max():
    slope = np.array([0.0, 0.5, 3.0, 30.0, 90.0])
    got = hy.q_perch_max(slope)
    assert got.tolist() == [1.0e-5 * math.sin(float(v) * (math.pi / 180.0)) for v in slope]
    assert got[0] == 0.0 and got[4] == 1.0e-5
    e = hy.water_balance_error(100.0, 101.0, 4000.0, 3999.5, 1e-3, 0.0, 2e-4, 0.0, 1e-4, 0.0, 5e-4, DT, qflx_drain_perched=3e-5)
    assert e == (101.0 + 3999.5) - (100.0 + 4000.0) - (1e-3 + 0.0 - ((1e-4 + 0.0 + 5e-4) + 3e-5) - 2e-4 - 0.0) * DT
    assert hy.water_balance_error(100.0, 101.0, 4000.0, 3999.5, 1e-3, 0.0, 2e-4, 0.0, 1e-4, 0.0, 5e-4, DT) == \
        (101.0 + 3999.5) - (100.0 + 4000.0) - (1e-3 + 0.0 - (1e-4 + 0.0 + 5e-4) - 2e-4 - 0.0) * DT


def test_header_constants_and_symbols():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    enum = dict(re.findall(r"(ELMK_HYDF_[A-Z0-9_]+) = (\d+)", h))
    want = {"Q_PERCH_MAX": hy.Q_PERCH_MAX, "FROST_TABLE": hy.FROST_TABLE, "ZWT_PERCHED": hy.ZWT_PERCHED,
            "QFLX_DRAIN_PERCHED": hy.QFLX_DRAIN_PERCHED, "NROWS": hy.FROST_NROWS}
    assert {k: int(enum["ELMK_HYDF_" + k]) for k in want} == want and st.HYDF_NROWS == hy.FROST_NROWS == 4
    assert int(re.search(r"ELMK_HYD_NROWS = (\d+)", h).group(1)) == hy.NROWS == 23
    for name in ("enable", "read", "clear"):
        assert f"elmk_soil_hydrology_frost_{name}" in L.SIGNATURES and re.search(rf"\bint elmk_soil_hydrology_frost_{name}\(", h)
        assert hasattr(st.ELMState, f"soil_hydrology_frost_{name}")
    assert hasattr(st.ELMState, "soil_hydrology_frost_rows")
    assert "tfrz = 273.15" in h and "sat_lev = 0.9" in h and "perched and frost tables" not in h
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_soil_hydrology.hip")).read()
    for name, v in (("TFRZ", hy.TFRZ), ("SAT_LEV", hy.SAT_LEV)):
        m = re.search(rf"HY_{name} = (-?[0-9.e+-]+)", k)
        assert m and float(m.group(1)) == v, name
