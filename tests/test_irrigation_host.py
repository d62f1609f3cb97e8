"""Irrigation on the host (include/elmk.h "irrigation"): irrigation.step, the restatement the device stage (k_irrigation.hip) follows.
The apply step against the oracle's ground_flux (pinned to the reference's) bit for bit; the schedule, the time of day and the window's
step count by hand; the check on hand-built columns against the formula written out here; and the physics of one window on a dry
crop column stepped with hydrology.step: the water applied is the deficit measured, the root zone gets wetter, the closed budget takes
the term.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests.hydrology_cases import CLOSURE_BOUND, column, water_mass
from tests.irrigation_cases import CHAIN_STEPS, chain_tod, generated, rate_by_hand, smpso_of
from tests.support import ROOT, bits

DT = 1800.0
SMPSO = -66000.0


# ---- 1. the apply step against the reference's ground_flux --------------------------------------------------------------------------
def test_apply_equals_ground_flux_with_the_term():
    """qflx_rain_grnd and qflx_snwcp_liq as the oracle's seven wrappers leave them (qflx_irrig hardwired to 0), then A of
    irrigation.step, against elmo_ch_ground_flux called with the nonzero qflx_irrig on the same inputs: bit for bit, on capped and
    uncapped columns, frac_veg_nosno 0 and 1, a column whose precipitation term is -0.0, and q = 0."""
    from oracle import oracle as O
    from tests import helpers as H

    n = 96
    cols, scal, soil = synth.make_state(st.field_table() if os.path.exists(L.LIB_PATH) else H.field_table_from_oracle(), n, tier="B", seed=41)
    c = np.arange(n)
    cols["do_capsnow"][:] = (c % 3 == 0).astype(np.int32)
    cols["forc_rain"][c % 8 == 5] = -0.0  # bare columns below take forc_rain itself as the precipitation term
    cols["forc_rain"][c % 8 == 6] = 0.0
    fvn_bare = (c % 8 == 5) | (c % 8 == 6) | (c % 8 == 7)
    cols["frac_veg_nosno"][fvn_bare] = 0
    S = H.oracle_state(cols, scal, soil)
    pre = {k: np.array(S.fields[k]) for k in ("h2ocan", "forc_rain", "forc_snow", "elai", "esai", "frac_veg_nosno", "do_capsnow")}
    S.timestep7(DT)
    assert np.array_equal(S.fields["do_capsnow"], pre["do_capsnow"]) and np.array_equal(S.fields["frac_veg_nosno"], pre["frac_veg_nosno"])
    assert set(zip(pre["do_capsnow"].tolist(), pre["frac_veg_nosno"].tolist())) == {(0, 0), (0, 1), (1, 0), (1, 1)}

    lib = O.lib().lib
    land = (C.c_int * 5)(*(S.scalars[k] for k in ("ltype", "ctype", "vtype", "urbpoi", "lakpoi")))
    dbl = C.c_double

    def ground_flux(i, q):
        h2ocan, drip, ts, tr, fs, fr = (dbl(float(pre["h2ocan"][i])), dbl(), dbl(), dbl(), dbl(), dbl())
        fvn, rain, snow = int(pre["frac_veg_nosno"][i]), dbl(float(pre["forc_rain"][i])), dbl(float(pre["forc_snow"][i]))
        lib.elmo_ch_interception(land, fvn, rain, snow, dbl(float(S.scalars["dewmx"])), dbl(float(pre["elai"][i])), dbl(float(pre["esai"][i])),
                                 dbl(DT), C.byref(h2ocan), C.byref(drip), C.byref(ts), C.byref(tr), C.byref(fs), C.byref(fr))
        out = [dbl() for _ in range(4)]
        lib.elmo_ch_ground_flux(land, int(pre["do_capsnow"][i]), fvn, rain, snow, dbl(q), drip, ts, tr, fs, fr, *(C.byref(o) for o in out))
        return out[0].value, out[3].value  # qflx_snwcp_liq, qflx_rain_grnd

    # the recomputation with the hardwired zero is what the wrappers stored
    zero = np.array([ground_flux(i, 0.0) for i in range(n)])
    assert bits(zero[:, 0]) == bits(S.fields["qflx_snwcp_liq"]) and bits(zero[:, 1]) == bits(S.fields["qflx_rain_grnd"])
    # a -0.0 precipitation term reaches ground_flux: the stored value is +0.0 there (prec_rain + 0.0)
    neg = (c % 8 == 5)
    assert np.signbit(pre["forc_rain"][neg]).all() and not np.signbit(zero[neg, 0] + zero[neg, 1]).any()

    q = np.where(c % 4 == 3, 0.0, 1.0e-4 * (1.0 + c / 7.0))  # q = 0 in a quarter of the columns
    rows = np.zeros((ir.NROWS, n))
    rows[ir.RATE], rows[ir.NLEFT] = q, 3.0
    fields = {k: np.array(S.fields[k]) for k in ir.READS}
    hit = {}
    out, rows_out = ir.step(fields, rows, np.full(n, -1, np.int32), DT, 0, SMPSO, hit=hit)
    want = np.array([ground_flux(i, float(q[i])) for i in range(n)])
    assert bits(out["qflx_snwcp_liq"]) == bits(want[:, 0]) and bits(out["qflx_rain_grnd"]) == bits(want[:, 1])
    assert hit["apply_capped"] > 0 and hit["apply_uncapped"] > 0 and hit["apply_zero"] > 0 and hit["not_irrigated"] == n
    assert bits(rows_out[ir.QFLX_IRRIG]) == bits(q) and (rows_out[ir.NLEFT] == 2.0).all() and bits(rows_out[ir.RATE]) == bits(q)
    assert (want[neg & (q > 0), :].sum(axis=1) == q[neg & (q > 0)]).all()  # -0.0 + q == +0.0 + q == q


# ---- 2. schedule, time of day, steps per day ----------------------------------------------------------------------------------------
def test_schedule_time_of_day_and_steps_per_day():
    assert [ir.steps_per_day(dt) for dt in (1800, 3600, 7000, 14400, 86400, 1)] == [8, 4, 3, 1, 1, 14400]
    for bad in (0, 86401, 1800.5, -1):
        with pytest.raises(ValueError):
            ir.steps_per_day(bad)
    lon = np.array([-180.0, -0.002, 0.0, 179.999, 15.0, -15.0, 360.0, 7.5])
    assert ir.schedule(np.ones(8, bool), lon).tolist() == [43200, 0, 0, 43200, 3600, 82800, 0, 1800]
    # half-second ties go away from zero: 1.5 s -> 2, -1.5 s -> -2, 0.5 s -> 1, -0.5 s -> -1
    ties = np.array([1.5, -1.5, 0.5, -0.5, 2.5]) * ir.DEGPSEC
    assert (ties / ir.DEGPSEC == np.array([1.5, -1.5, 0.5, -0.5, 2.5])).all()
    assert ir.schedule(np.ones(5, bool), ties).tolist() == [2, 86398, 1, 86399, 3]
    s = ir.schedule(np.array([True, False, True]), np.array([10.0, 10.0, -170.0]))
    assert s.dtype == np.int32 and s.tolist() == [2400, -1, 45600]
    assert ir.time_of_day(1.0, 0) == 0 and ir.time_of_day(14.875 + 1800.0 / 86400.0, 13) == 77400 and ir.time_of_day(15.0, 14) == 0
    assert ir.time_of_day(15.0, 13) == 0 and ir.time_of_day(182.25, 181) == 21600  # (a whole day past reduces)
    # every longitude on a 7.5-degree grid checks in exactly one step of a 1800 s day
    sched = ir.schedule(np.ones(48, bool), -180.0 + 7.5 * np.arange(48))
    count = np.zeros(48, int)
    for k in range(48):
        count += ir.seconds_since_start(sched, 1800 * k) < 1800
    assert (count == 1).all()


# ---- 3. the check on hand-built columns ---------------------------------------------------------------------------------------------
def _fields(ncol, sat=0.3, **over):
    """ncol uniform loam columns on ELM's grid (hydrology_cases.column: watsat 0.45, sucsat 200 mm, bsw 5, no ice), fifteen soil
    layers of which the ten active ones carry water and roots; every field irrigation.step and hydrology.step read.  Vegetated, leafy,
    stressed (btran 0.3), thawed (280 K), snow-free, uncapped."""
    col = column(sat=sat)
    dz = np.array(col["dz"] + [1.0] * 5)
    zi = np.concatenate([[0.0], np.cumsum(dz)])
    f = {}
    lev = lambda v: np.concatenate([np.zeros(5), v])  # noqa: E731
    f["dz"] = np.tile(lev(dz), (ncol, 1))
    f["zsoi"] = np.tile(lev(0.5 * (zi[1:] + zi[:-1])), (ncol, 1))
    f["zisoi"] = np.tile(np.concatenate([np.zeros(5), zi]), (ncol, 1))
    for k, v in (("watsat", 0.45), ("sucsat", 200.0), ("bsw", 5.0), ("eff_porosity", 0.45)):
        f[k] = np.full((ncol, 15), v)
    liq = sat * 0.45 * dz * 1.0e3
    f["h2osoi_liq"] = np.tile(lev(liq), (ncol, 1))
    f["h2osoi_ice"] = np.zeros((ncol, 20))
    f["h2osoi_vol"] = np.full((ncol, 15), sat * 0.45)
    f["t_soisno"] = np.full((ncol, 20), 280.0)
    root = np.zeros(15)
    root[:8] = [0.25, 0.2, 0.15, 0.12, 0.1, 0.08, 0.06, 0.04]
    f["rootfr"] = np.tile(root, (ncol, 1))
    f["qflx_rootsoi"] = np.zeros((ncol, 15))
    for k in ("h2osfc", "frac_h2osfc", "frac_sno_eff", "qflx_top_soil", "qflx_evap_grnd", "qflx_ev_soil", "qflx_ev_h2osfc", "qflx_dew_grnd",
              "qflx_dew_snow", "qflx_sub_snow", "qflx_rain_grnd", "qflx_snwcp_liq", "h2ocan", "h2osno", "forc_rain", "forc_snow",
              "qflx_evap_tot", "qflx_snwcp_ice"):
        f[k] = np.zeros(ncol)
    f["snl"] = np.zeros(ncol, np.int32)
    f["do_capsnow"] = np.zeros(ncol, np.int32)
    f["frac_veg_nosno"] = np.ones(ncol, np.int32)
    f["elai"] = np.full(ncol, 2.0)
    f["btran"] = np.full(ncol, 0.3)
    for k, v in over.items():
        f[k] = v
    return f


_rate_by_hand = rate_by_hand  # (the formula written out: tests/irrigation_cases.py, shared with the edge tier's host tests)


CASES = ("plain", "frozen_top", "frozen_layer_3", "rootless_layers", "wetter_than_target", "btran_at_threshold", "btran_just_below",
         "no_lai", "no_veg", "not_irrigated", "nan_sucsat", "off_clock", "stale_rate")


def test_the_check_on_hand_built_columns():
    n = len(CASES)
    k = {name: i for i, name in enumerate(CASES)}
    f = _fields(n)
    f["t_soisno"][k["frozen_top"], 5] = 273.15
    f["t_soisno"][k["frozen_layer_3"], 5 + 3] = 270.0
    f["rootfr"][k["rootless_layers"], [0, 2, 5]] = 0.0
    f["h2osoi_liq"][k["wetter_than_target"], 5:15] = 0.999 * 0.45 * f["dz"][0, 5:15] * 1.0e3
    f["btran"][k["btran_at_threshold"]] = 0.999999
    f["btran"][k["btran_just_below"]] = np.nextafter(0.999999, 0.0)
    f["elai"][k["no_lai"]] = 0.0
    f["frac_veg_nosno"][k["no_veg"]] = 0
    f["sucsat"][k["nan_sucsat"], 2] = np.nan
    sched = np.zeros(n, np.int32)
    sched[k["not_irrigated"]] = -1
    sched[k["off_clock"]] = 1800  # half an hour further east: its step was the one before
    rows = np.zeros((ir.NROWS, n))
    rows[ir.RATE, k["stale_rate"]], rows[ir.NLEFT, k["stale_rate"]] = 7.0e-4, 0.0  # an expired window: nothing applied, then a new one
    rows[ir.RATE, k["off_clock"]], rows[ir.NLEFT, k["off_clock"]] = 3.0e-4, 7.0  # inside its window: applies, does not check
    hit = {}
    out, got = ir.step(f, rows, sched, DT, 21600, SMPSO, hit=hit)
    want_rate = np.zeros(n)
    want_nleft = np.zeros(n)
    checking = [name for name in CASES if name not in ("btran_at_threshold", "no_lai", "no_veg", "not_irrigated", "off_clock")]
    for name in checking:
        want_nleft[k[name]] = 8.0
        want_rate[k[name]] = _rate_by_hand(f, k[name], {"frozen_top": 0, "frozen_layer_3": 3}.get(name, 15), DT)
    want_rate[k["off_clock"]], want_nleft[k["off_clock"]] = 3.0e-4, 6.0
    assert np.isnan(want_rate[k["nan_sucsat"]])
    assert bits(got[ir.NLEFT]) == bits(want_nleft)
    assert bits(got[ir.RATE]) == bits(np.where(np.isnan(want_rate), np.float64(np.nan), want_rate))
    assert got[ir.RATE].view(np.uint64)[k["nan_sucsat"]] == 0x7FF8000000000000
    assert got[ir.RATE, k["frozen_top"]] == 0.0 and not np.signbit(got[ir.RATE, k["frozen_top"]])  # +0.0, and the window is set all the same
    assert got[ir.RATE, k["wetter_than_target"]] == 0.0
    assert 0.0 < got[ir.RATE, k["frozen_layer_3"]] < got[ir.RATE, k["rootless_layers"]] < got[ir.RATE, k["plain"]]
    assert got[ir.RATE, k["btran_just_below"]] == got[ir.RATE, k["plain"]] == got[ir.RATE, k["stale_rate"]]
    # this step applied only where a window was open
    want_q = np.zeros(n)
    want_q[k["off_clock"]] = 3.0e-4
    assert bits(got[ir.QFLX_IRRIG]) == bits(want_q) and bits(out["qflx_rain_grnd"]) == bits(want_q) and not out["qflx_snwcp_liq"].any()
    assert {b for b in ir.BRANCHES if not hit.get(b)} == {"apply_capped", "apply_zero"}, hit  # (those two: test_apply_equals_ground_flux)
    # fp32 state: the sum is rounded once to the stored type
    f32 = {key: (v.astype(np.float32) if v.dtype == np.float64 else v) for key, v in f.items()}
    f32["qflx_rain_grnd"] = np.full(n, 0.1, np.float32)
    o32, _ = ir.step(f32, rows, sched, DT, 21600, SMPSO)
    assert o32["qflx_rain_grnd"].dtype == np.float32
    assert o32["qflx_rain_grnd"][k["off_clock"]] == np.float32(np.float64(np.float32(0.1)) + 3.0e-4)
    # the inputs are only read
    f2 = _fields(n)
    before = {key: v.copy() for key, v in f2.items()}
    ir.step(f2, rows, sched, DT, 21600, SMPSO)
    assert all(bits(f2[key]) == bits(before[key]) for key in f2)


# ---- 4. the physics of one window ---------------------------------------------------------------------------------------------------
def test_one_window_on_a_dry_crop_column():
    """Four dry columns at four longitudes through a day of 1800 s steps: irrigation.step, then hydrology.step with the water on the
    ground as qflx_top_soil (no snow, no canopy, no ponding: snow_hydrology hands qflx_rain_grnd on unchanged), then the closed budget.
    The water applied over the window equals the deficits summed at check time; the root zone gets wetter; ERRH2O takes the term."""
    n = 4
    f = _fields(n, sat=0.25)
    sched = ir.schedule(np.ones(n, bool), np.array([0.0, 7.5, -15.0, 90.0]))
    rows = np.zeros((ir.NROWS, n))
    hyd = np.zeros((hy.NROWS, n))
    hyd[hy.ZWT], hyd[hy.WA] = 6.0, 4000.0
    hyd[hy.HKSAT:hy.HKSAT + hy.N] = 0.005
    hyd[hy.H2OSFC_THRESH], hyd[hy.K_WET] = 5.0, 0.05
    root0 = (f["h2osoi_liq"][:, 5:13]).sum(axis=1)
    deficit_mm = np.zeros(n)
    applied = np.zeros(n)
    worst = 0.0
    for s in range(48):
        tod = 1800 * s
        out, new = ir.step(f, rows, sched, DT, tod, SMPSO)
        started = (new[ir.NLEFT] == 8.0) & (rows[ir.NLEFT] == 0.0)
        for c in np.nonzero(started)[0]:
            deficit_mm[c] = _rate_by_hand(f, c, 15, DT) * (DT * 8)
        rows = new
        f.update(out)
        q = rows[ir.QFLX_IRRIG]
        applied = applied + q * DT
        f["qflx_top_soil"] = f["qflx_rain_grnd"].copy()
        f["dtbegin_column_h2o"] = water_mass(f)
        wb = hy.water_balance_begin(f, hyd)
        out_h, hyd = hy.step(f, hyd, DT)
        f.update(out_h)
        with_term = hy.water_balance_end(f, hyd, wb, DT, qflx_irrig=q)
        without = hy.water_balance_end(f, hyd, wb, DT)
        ref = hy.water_balance_error(f["dtbegin_column_h2o"], water_mass(f), wb[hy.WB_BEGWB] - f["dtbegin_column_h2o"], hyd[hy.WA], f["forc_rain"],
                                     f["forc_snow"], f["qflx_evap_tot"], f["qflx_snwcp_ice"], hyd[hy.QFLX_SURF], hyd[hy.QFLX_H2OSFC_SURF],
                                     hyd[hy.QFLX_DRAIN], DT, qflx_irrig=q)
        assert np.array_equal(with_term[hy.WB_ERRH2O], ref)
        assert bits(hy.water_balance_end(f, hyd, wb, DT, qflx_irrig=np.zeros(n))[hy.WB_ERRH2O]) != bits(with_term[hy.WB_ERRH2O]) or not q.any()
        # the term is q * dt of the budget, to the rounding of a 5000 mm water mass
        assert np.abs((without[hy.WB_ERRH2O] - with_term[hy.WB_ERRH2O]) - q * DT).max() <= 16 * 2.0 ** -53 * with_term[hy.WB_ENDWB].max()
        worst = max(worst, float(np.abs(with_term[hy.WB_ERRH2O]).max()))
        f["qflx_rain_grnd"] = np.zeros(n)  # canopy_hydrology stores it anew every step
    print(f"one window: applied {applied.tolist()} mm, deficits {deficit_mm.tolist()} mm, max |ERRH2O| with the term {worst:.3e} mm")
    assert (deficit_mm > 1.0).all()
    assert np.abs(applied - deficit_mm).max() <= 1.0e-12 * deficit_mm.max()
    assert (rows[ir.NLEFT] == 0.0).all()  # every window has run out by the end of the day
    assert (f["h2osoi_liq"][:, 5:13].sum(axis=1) > root0 + 1.0).all()  # (the rest ran off: the rate exceeds what this loam takes in)
    assert worst <= CLOSURE_BOUND
    # the defaults reproduce the un-irrigated bits
    assert bits(hy.water_balance_end(f, hyd, wb, DT)) == bits(hy.water_balance_end(f, hyd, wb, DT, qflx_irrig=None))


# ---- the header, the bindings and the restart kinds ---------------------------------------------------------------------------------
def test_header_constants_and_symbols():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert re.search(r"#define ELMK_RUN_IRRIGATION 128\b", h) and st.RUN_IRRIGATION == 128
    assert "enum { ELMK_IRR_RATE = 0, ELMK_IRR_NLEFT = 1, ELMK_IRR_QFLX_IRRIG = 2 };" in h
    assert (ir.RATE, ir.NLEFT, ir.QFLX_IRRIG) == (st.IRR_RATE, st.IRR_NLEFT, st.IRR_QFLX_IRRIG) == (0, 1, 2)
    assert "ELMK_ROWS_IRRIGATION = 4, ELMK_ROWS_NFAMILY = 5" in h and st.ROWS_IRRIGATION == R.ROWS_IRRIGATION == 4
    assert st.ROW_FAMILIES["irrigation"] == 4
    assert "ELMK_RESTART_IRRIGATION = 6" in h and R.IRRIGATION_SECTION == 6
    assert "#define ELMK_RESTART_VERSION_IRRIGATION 5u" in h and R.VERSION_IRRIGATION == 5 and R.OPTIONAL[-1] == (6, 5)
    for name in ("enable", "init", "read", "clear"):
        assert f"int elmk_irrigation_{name}(" in h and f"elmk_irrigation_{name}" in L.SIGNATURES
    assert "int elmk_irrigation(elmk_ctx *ctx, double dt, int tod_seconds);" in h and "elmk_irrigation" in L.SIGNATURES
    assert R.row_field(st.ROWS_IRRIGATION, ir.QFLX_IRRIG) == 0x40000000 + (4 << 16) + 2
    for doc in ("include/elmk.h", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert not re.search(r"[Oo]ut of scope:[^.]*\birrigation,", text), doc


def test_the_generated_tier_takes_every_branch():
    """The oracle's seven wrappers and irrigation.step, fifty chained steps on 600 generated columns: every branch of A and B is taken,
    and in one 64-column wave of one step some columns check, some apply and some do neither."""
    from tests import helpers as H

    n = 600
    cols, scal, soil, sched = generated(n, 900)
    S = H.oracle_state(cols, scal, soil)
    rows = np.zeros((ir.NROWS, n))
    smpso = smpso_of(cols["vtype"])
    hit = {}
    mixed = 0
    for s in range(CHAIN_STEPS):
        S.timestep7(DT)
        before = rows
        out, rows = ir.step({k: np.array(S.fields[k]) for k in ir.READS}, rows, sched, DT, chain_tod(s), smpso, hit=hit)
        for k, v in out.items():
            S.fields[k][...] = v
        checked = (rows[ir.NLEFT] == 8.0)[:64]
        applied = (before[ir.NLEFT] > 0.0)[:64]
        mixed += bool(checked.any() and applied.any() and (~checked & ~applied).any())
    print("census:", hit, "steps with a mixed first wave:", mixed)
    assert all(hit.get(b, 0) > 0 for b in ir.BRANCHES), {b for b in ir.BRANCHES if not hit.get(b)}
    assert mixed > 0
    assert np.isfinite(rows).all()


# ---- restart images of version 5 ----------------------------------------------------------------------------------------------------
def _image(gcol0, n, hydrology, seed):
    rng = np.random.default_rng(seed)
    h = np.zeros((), R.HEADER)
    h["magic"], h["real_bytes"], h["schema_hash"], h["gcol0"], h["ncols"] = R.MAGIC, 8, 1234, gcol0, n
    kinds = [(R.FIELD, 3, 2)] + ([(R.HYDROLOGY_SECTION, hy.ZWT, 1), (R.HYDROLOGY_SECTION, hy.WA, 1)] if hydrology else [])
    kinds += [(R.IRRIGATION_SECTION, ir.RATE, 1), (R.IRRIGATION_SECTION, ir.NLEFT, 1)]
    sec = np.zeros(len(kinds), R.SECTION)
    data = []
    for i, (kind, ident, nlev) in enumerate(kinds):
        d = rng.standard_normal((nlev, n))
        sec[i] = (kind, ident, nlev, 0, n, 0, R.checksum(d, gcol0))
        data.append(d)
    return R.build(h, np.zeros(0, R.ENTRY), sec, data), data


@pytest.mark.parametrize("hydrology", [False, True], ids=["irrigation", "hydrology+irrigation"])
def test_restart_version_5_parse_merge_slice(hydrology):
    a, da = _image(0, 96, hydrology, 1)
    b, db = _image(96, 64, hydrology, 2)
    pa = R.verify(a)
    assert int(pa["header"]["version"]) == 5
    kinds = [int(k) for k in pa["sections"]["kind"]]
    assert kinds[-2:] == [R.IRRIGATION_SECTION] * 2 and (R.HYDROLOGY_SECTION in kinds) == hydrology
    assert [int(i) for i in pa["sections"]["id"][-2:]] == [ir.RATE, ir.NLEFT]
    m = R.merge([a, b])
    pm = R.verify(m)
    assert int(pm["header"]["version"]) == 5 and int(pm["header"]["ncols"]) == 160
    assert np.array_equal(np.asarray(pm["data"][-1]).reshape(1, -1), np.concatenate([da[-1], db[-1]], axis=1))
    s = R.slice(m, 96, 64)
    ps = R.verify(s)
    assert int(ps["header"]["version"]) == 5 and int(ps["header"]["gcol0"]) == 96
    for got, want in zip(ps["data"], db):
        assert np.array_equal(np.asarray(got).reshape(want.shape), want)
    bad = a.copy()  # the sections under an older version
    hdr = np.frombuffer(bad[:R.HEADER.itemsize].tobytes(), R.HEADER).copy()
    hdr["version"] = 4
    bad[:R.HEADER.itemsize] = np.frombuffer(hdr.tobytes(), np.uint8)
    with pytest.raises(R.RestartError):
        R.parse(bad)
