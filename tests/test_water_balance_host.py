"""The water balance on the host (include/elmk.h "water balance"): hydrology.water_balance_begin / water_balance_end / water_balance_reduce,
the restatement the device stage (k_water_balance.hip) follows, against hydrology.water_balance_error on the six-step host chain,
hand-computed columns for SOILWATER_10CM and numpy for the reduction and the census.  No GPU."""
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import diagnostics as D
from elmkernels_amd import hydrology as hy
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from tests.hydrology_cases import CHAIN_STEPS, DT, generated_frost, water_mass
from tests.support import ROOT

N = hy.N


def wb_host_chain(cols, scal, soil, rows, frost, nsteps=CHAIN_STEPS, dt=DT):
    """hydrology_cases.host_chain (frost: test_frost_table_host.frost_host_chain) with W0 after init_timestep and W1 - W6 after the
    stage.  Per step: the rows of the feature, the same without W3's last term, hydrology.water_balance_error of the step and
    qflx_snwcp_liq."""
    from tests import helpers as H

    S = H.oracle_state(cols, scal, soil)
    rows = rows.copy()
    wb = None
    per_step = []
    for _ in range(nsteps):
        S.init_timestep()
        wb = hy.water_balance_begin(S.fields, rows, wb)
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
        f = {k: np.array(S.fields[k]) for k in hy.WB_READS + ("dtbegin_column_h2o",)}
        without = hy.water_balance_end(f, rows, wb, dt, frost=frost, snwcp_liq_term=False)
        wb = hy.water_balance_end(f, rows, wb, dt, frost=frost)
        ref = hy.water_balance_error(f["dtbegin_column_h2o"], water_mass(f), wa_beg, rows[hy.WA], f["forc_rain"], f["forc_snow"],
                                     f["qflx_evap_tot"], f["qflx_snwcp_ice"], rows[hy.QFLX_SURF], rows[hy.QFLX_H2OSFC_SURF],
                                     rows[hy.QFLX_DRAIN], dt, qflx_drain_perched=None if frost is None else frost[hy.QFLX_DRAIN_PERCHED])
        per_step.append((wb.copy(), without, ref, f["qflx_snwcp_liq"].astype(np.float64)))
    return per_step


@pytest.fixture(scope="module")
def chain_inputs():
    return generated_frost(1001, 77, full=True, chain=True)


@pytest.mark.parametrize("frost", [False, True], ids=["plain", "frost"])
def test_errh2o_is_the_closed_budget_of_the_host_chain(chain_inputs, frost):
    """On every column where snow capping removes no liquid the stage's ERRH2O is hydrology.water_balance_error, value for value, in
    all six steps.  On the capped-snow columns (qflx_snwcp_liq != 0) |ERRH2O| is printed with and without W3's last term: a measurement,
    recorded in DESIGN.md section 21."""
    cols, scal, soil, rows, fr = chain_inputs
    steps = wb_host_chain(cols, scal, soil, rows, fr if frost else None)
    ncapped = 0
    for s, (wb, without, ref, snwcp_liq) in enumerate(steps):
        same = snwcp_liq == 0.0
        assert same.sum() > 0.5 * same.size
        assert np.array_equal(wb[hy.WB_ERRH2O][same], ref[same])
        assert np.isfinite(wb).all()
        cap = ~same
        ncapped += int(cap.sum())
        if cap.any():
            a, b = np.abs(wb[hy.WB_ERRH2O][cap]), np.abs(without[hy.WB_ERRH2O][cap])
            print(f"step {s} frost={frost}: {int(cap.sum())} capped-snow columns; |ERRH2O| with the W3 term median {np.median(a):.6g} "
                  f"max {a.max():.6g}; without it median {np.median(b):.6g} max {b.max():.6g}")
    print(f"frost={frost}: {ncapped} capped-snow column steps in the chain")


# ---- W5, W6 by hand ---------------------------------------------------------------------------------------------------------------
def _one_column(zi, liq, ice):
    """One column whose ten active layers have the interfaces zi[0 .. 10] (zi[0] the surface), dz = their differences and the given
    liq, ice; the bedrock levels hold 1000 mm each, which W5 and W6 must never see."""
    f = {k: np.zeros(1) for k in ("h2ocan", "h2osno", "h2osfc", "qflx_snwcp_liq", "forc_rain", "forc_snow", "qflx_evap_tot", "qflx_snwcp_ice",
                                  "dtbegin_column_h2o")}
    f["h2osoi_liq"], f["h2osoi_ice"] = np.zeros((1, 20)), np.zeros((1, 20))
    f["h2osoi_liq"][0, 5:15], f["h2osoi_ice"][0, 5:15] = liq, ice
    f["h2osoi_liq"][0, 15:] = 1000.0
    f["h2osoi_ice"][0, 15:] = 1000.0
    f["zisoi"] = np.zeros((1, 21))
    f["zisoi"][0, 5:16] = zi
    f["dz"] = np.ones((1, 20))
    f["dz"][0, 5:15] = [zi[j + 1] - zi[j] for j in range(N)]
    return f


def _end(f):
    rows = np.zeros((hy.NROWS, 1))
    return hy.water_balance_end(f, rows, hy.water_balance_begin(f, rows), DT)


def test_soilwater_10cm_by_hand():
    liq = [float(j + 1) for j in range(N)]
    ice = [0.5 * (j + 1) for j in range(N)]
    tot = [liq[j] + ice[j] for j in range(N)]
    # a layer ending exactly at 0.1 m: layers 0 .. 2 whole, nothing of layer 3 (zi[j-1] < 0.1 is false for it)
    zi = [0.0, 0.02, 0.05, 0.1, 0.2, 0.4, 0.8, 1.4, 2.3, 3.8, 5.0]
    wb = _end(_one_column(zi, liq, ice))
    assert wb[hy.WB_SOILWATER_10CM, 0] == ((0.0 + tot[0]) + tot[1]) + tot[2]
    # a layer straddling it: ELM's grid, layer 3 spans 0.0906 .. 0.1655
    zi = [0.0, 0.0175, 0.0451, 0.0906, 0.1655, 0.2891, 0.4929, 0.8289, 1.3828, 2.2961, 3.8019]
    f = _one_column(zi, liq, ice)
    wb = _end(f)
    dz3 = float(f["dz"][0, 8])
    assert wb[hy.WB_SOILWATER_10CM, 0] == (((0.0 + tot[0]) + tot[1]) + tot[2]) + tot[3] * ((0.1 - 0.0906) / dz3)
    # zi[0] > 0.1: only the fraction 0.1 / dz of the top layer
    zi = [0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0, 4.5]
    f = _one_column(zi, liq, ice)
    wb = _end(f)
    assert wb[hy.WB_SOILWATER_10CM, 0] == 0.0 + tot[0] * ((0.1 - 0.0) / 0.25)
    # W5: the ten active layers in ascending order, the bedrock levels never
    want_l, want_i = 0.0, 0.0
    for j in range(N):
        want_l, want_i = want_l + liq[j], want_i + ice[j]
    assert wb[hy.WB_TOTSOILLIQ, 0] == want_l and wb[hy.WB_TOTSOILICE, 0] == want_i
    # W1 / W2 take all twenty levels
    assert wb[hy.WB_ENDWB, 0] == water_mass(f)[0] and wb[hy.WB_ENDWB, 0] > 10000.0


def test_runoff_and_error_by_hand():
    f = _one_column([0.1 * j for j in range(11)], [10.0] * N, [0.0] * N)
    f["dtbegin_column_h2o"][:] = 10100.0
    f["forc_rain"][:], f["forc_snow"][:], f["qflx_evap_tot"][:], f["qflx_snwcp_ice"][:] = 1e-3, 2e-4, 3e-4, 1e-5
    f["qflx_snwcp_liq"][:] = 4e-5
    rows = np.zeros((hy.NROWS, 1))
    rows[hy.WA], rows[hy.QFLX_SURF], rows[hy.QFLX_H2OSFC_SURF], rows[hy.QFLX_DRAIN] = 4000.0, 1e-4, 2e-5, 5e-4
    fr = np.zeros((hy.FROST_NROWS, 1))
    fr[hy.QFLX_DRAIN_PERCHED] = 7e-5
    wb0 = hy.water_balance_begin(f, rows)
    assert wb0[hy.WB_BEGWB, 0] == 10100.0 + 4000.0
    rows[hy.WA] = 3999.0
    plain, frost = hy.water_balance_end(f, rows, wb0, DT), hy.water_balance_end(f, rows, wb0, DT, frost=fr)
    q = 1e-4 + 2e-5 + 5e-4
    assert plain[hy.WB_QRUNOFF, 0] == q + 4e-5 and frost[hy.WB_QRUNOFF, 0] == (q + 7e-5) + 4e-5
    endwb = float(water_mass(f)[0]) + 3999.0
    assert plain[hy.WB_ENDWB, 0] == endwb
    assert plain[hy.WB_ERRH2O, 0] == endwb - (10100.0 + 4000.0) - (1e-3 + 2e-4 - (q + 4e-5) - 3e-4 - 1e-5) * DT
    # a NaN is stored as the canonical quiet NaN
    f["h2osoi_liq"][0, 7] = -np.float64(np.nan)
    nan = hy.water_balance_end(f, rows, wb0, DT)
    for w in (hy.WB_ERRH2O, hy.WB_ENDWB, hy.WB_TOTSOILLIQ):
        assert nan[w].view(np.uint64)[0] == 0x7FF8000000000000


# ---- W7, W8 -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 131073])
def test_reduction_and_census(n):
    rng = np.random.default_rng(n)
    wb = rng.standard_normal((hy.WB_NROWS, n))
    wb[hy.WB_ERRH2O] *= 1.0e-9
    tol = float(np.median(np.abs(wb[hy.WB_ERRH2O])))
    mms, nbad, first = hy.water_balance_reduce(wb, tol)
    for i, k in enumerate((hy.WB_ERRH2O, hy.WB_QRUNOFF, hy.WB_ENDWB)):
        assert mms[i].tobytes() == D.reduce_min_max_sum(wb[k]).tobytes()
        assert mms[i, 0] == wb[k].min() and mms[i, 1] == wb[k].max() and abs(mms[i, 2] - wb[k].sum()) <= 1e-9 * np.abs(wb[k]).sum()
    bad = [c for c in range(n) if not abs(wb[hy.WB_ERRH2O, c]) <= tol]
    assert nbad == len(bad) and first == (bad[0] if bad else -1)
    # a NaN column is bad and makes min and max NaN; tol = 0 leaves only exact zeros good
    wb[hy.WB_ERRH2O, n // 2] = np.nan
    if n > 1:
        wb[hy.WB_ERRH2O, 0] = 0.0
    mms, nbad, first = hy.water_balance_reduce(wb, 0.0)
    assert np.isnan(mms[0, 0]) and np.isnan(mms[0, 1]) and np.isnan(mms[0, 2])
    want = np.count_nonzero(wb[hy.WB_ERRH2O] != 0.0)  # (NaN != 0.0)
    assert nbad == want and first == int(np.nonzero(wb[hy.WB_ERRH2O] != 0.0)[0][0])
    big = hy.water_balance_reduce(wb, 1.0e30)
    assert big[1] == 1 and big[2] == n // 2
    empty = hy.water_balance_reduce(np.zeros((hy.WB_NROWS, 0)), 1.0)
    assert empty[0].tolist() == [[np.inf, -np.inf, 0.0]] * 3 and empty[1:] == (0, -1)


# ---- constants, symbols, the restart encoding ---------------------------------------------------------------------------------------
def test_header_constants_and_symbols():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    enum = dict(re.findall(r"(ELMK_WB_[A-Z0-9_]+) = (\d+)", h))
    want = {"BEGWB": hy.WB_BEGWB, "ERRH2O": hy.WB_ERRH2O, "QRUNOFF": hy.WB_QRUNOFF, "ENDWB": hy.WB_ENDWB, "SOILWATER_10CM": hy.WB_SOILWATER_10CM,
            "TOTSOILLIQ": hy.WB_TOTSOILLIQ, "TOTSOILICE": hy.WB_TOTSOILICE, "NROWS": hy.WB_NROWS}
    assert {k: int(enum["ELMK_WB_" + k]) for k in want} == want and st.WB_NROWS == hy.WB_NROWS
    assert hy.WB_QRUNOFF == hy.WB_ERRH2O + 1 and hy.WB_ENDWB == hy.WB_ERRH2O + 2  # the reduction walks them as diag + k * ld
    assert re.search(r"#define ELMK_RUN_WATER_BALANCE 64\b", h) and st.RUN_WATER_BALANCE == 64
    fam = dict(re.findall(r"(ELMK_ROWS_[A-Z_]+) = (\d+)", h))
    assert [int(fam["ELMK_ROWS_" + k]) for k in ("ALT", "HYDROLOGY", "FROST", "WATER_BALANCE")] == [st.ROWS_ALT, st.ROWS_HYDROLOGY, st.ROWS_FROST,
                                                                                                 st.ROWS_WATER_BALANCE] == [0, 1, 2, 3]
    for name in ("water_balance_enable", "water_balance_begin", "water_balance", "water_balance_read", "water_balance_clear", "run_water_balance",
                 "column_history_add_row", "gridded_history_add_row"):
        assert "elmk_" + name in L.SIGNATURES and re.search(rf"^int elmk_{name}\(", h, re.M), name
        assert hasattr(st.ELMState, name.replace("column_", "")), name
    assert re.search(r"#define ELMK_RESTART_ROW_BASE 0x40000000\b", h) and R.ROW_BASE == 0x40000000
    assert R.row_field(st.ROWS_WATER_BALANCE, hy.WB_QRUNOFF) == 0x40000000 + (3 << 16) + 2
    assert R.entry_row(R.row_field(2, 3)) == (2, 3) and R.entry_row(17) is None
    assert "hydrology.water_balance_error is the closed budget" not in h
    d = open(os.path.join(ROOT, "include", "elmk_restart.def")).read()
    assert "0x40000000 + (family << 16) + which" in d


def test_row_entries_survive_merge_and_slice():
    """An image whose history entries are over feature rows: restart.merge and restart.slice carry the entry table and the one-level
    accumulator sections as they carry every entry."""
    def image(gcol0, n, seed):
        rng = np.random.default_rng(seed)
        h = np.zeros((), R.HEADER)
        h["magic"], h["real_bytes"], h["schema_hash"], h["gcol0"], h["ncols"] = R.MAGIC, 8, 99, gcol0, n
        h["tape_count"][0] = 3
        ent = np.zeros(2, R.ENTRY)
        ent[0] = (0, R.row_field(st.ROWS_WATER_BALANCE, hy.WB_QRUNOFF), 0, 0, 0)
        ent[1] = (0, R.row_field(st.ROWS_HYDROLOGY, hy.ZWT), 2, 0, 0)
        kinds = [(R.FIELD, 3, 2), (R.HISTORY, 0, 1), (R.HISTORY, 1, 1), (R.HYDROLOGY_SECTION, hy.ZWT, 1), (R.HYDROLOGY_SECTION, hy.WA, 1)]
        sec, data = np.zeros(len(kinds), R.SECTION), []
        for i, (kind, ident, nlev) in enumerate(kinds):
            d = rng.standard_normal((nlev, n))
            sec[i] = (kind, ident, nlev, 0, n, 0, R.checksum(d, gcol0))
            data.append(d)
        return R.build(h, ent, sec, data), data

    a, da = image(0, 96, 1)
    b, db = image(96, 64, 2)
    m = R.verify(R.merge([b, a]))
    assert [R.entry_row(f) for f in m["entries"]["field"]] == [(st.ROWS_WATER_BALANCE, hy.WB_QRUNOFF), (st.ROWS_HYDROLOGY, hy.ZWT)]
    assert np.array_equal(m["data"][1], np.concatenate([da[1], db[1]], axis=1))
    s = R.verify(R.slice(R.merge([a, b]), 96, 64))
    assert s["entries"].tobytes() == m["entries"].tobytes() and np.array_equal(s["data"][2], db[2])
