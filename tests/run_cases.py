"""The cases of the multi-step run that the GPU tests share: the inputs (state, geography, forcing and phenology records), the step
schedule, the same steps driven through the existing calls ("stepwise": the atm_* and mlai .. mhbot fields uploaded from the same host
records before every step, elmk_solar_geometry, elmk_phenology, elmk_get_forcing, elmk_init_timestep, elmk_advance_physics, then
elmk_evaluate_conservation and elmk_error_summary after every step), the upload of the series, and the bit-for-bit assertions."""
import numpy as np

from elmkernels_amd import active_layer as al
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H
from tests.support import same

DT = 1800.0
SERIES = st.SERIES_FORCING + st.SERIES_PHENOLOGY
NREC = 10  # hourly forcing records
NSTEPS = 12  # half-hour steps: forcing slots 0 .. 6
IMAGE_CLASSES = (st.CLASS_PROGNOSTIC, st.CLASS_SURFACE)  # the field classes a restart image holds


def _inputs(n, seed, nrec=NREC, tier="B"):
    """State, geography, nrec hourly records per forcing stream and 12 months per phenology field, all [records, n]."""
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier=tier, seed=seed)
    lat, lon = synth.global_grid(n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    rec = {}
    for k in st.SERIES_FORCING:
        a, b = cols[k][:, 0], cols[k][:, 1]
        t = np.linspace(0.0, 1.0, nrec)[:, None]
        rec[k] = (1.0 - t) * a[None, :] + t * b[None, :] + 0.01 * np.abs(a)[None, :] * rng.standard_normal((nrec, n))
    # long-wave: both branches of ProcessFLDS (<= 50, >= 600) in some columns of some records
    m = rng.random((nrec, n))
    rec["atm_flds"] = np.where(m < 0.05, 30.0, np.where(m > 0.95, 700.0, rec["atm_flds"]))
    rec["atm_prec"] = np.where(rng.random((nrec, n)) < 0.3, 0.0, np.abs(rec["atm_prec"]))  # some dry records
    rec["atm_fsds"] = np.abs(rec["atm_fsds"])
    for k in st.SERIES_PHENOLOGY:
        base = cols[k][:, 0]
        rec[k] = np.abs(base[None, :] * (1.0 + 0.1 * rng.standard_normal((12, n))))
    return cols, scal, soil, lat, lon, rec


def schedule(nsteps=NSTEPS, slot0=0):
    """Half-hour steps from 21:00 of day 13: crosses midnight; the month bracket moves from (11, 0) to (0, 1) half way; distinct
    weights for every stream."""
    S = np.zeros(nsteps, st.RUN_STEP_DTYPE)
    for s in range(nsteps):
        ddoy = 13.875 + s * DT / 86400.0
        S[s]["decday"] = ddoy + 1.0
        S[s]["doy"] = int(ddoy)
        S[s]["forc_slot"] = slot0 + s // 2
        e = (s % 2) * 0.5 + 0.25
        w2 = np.clip(e + 0.03 * np.arange(8) - 0.1, 0.0, 1.0)
        S[s]["forc_wt2"] = w2
        S[s]["forc_wt1"] = 1.0 - w2
        if s < nsteps // 2:
            S[s]["month1"], S[s]["month2"], S[s]["month_wt1"] = 11, 0, 0.3 - 0.01 * s
        else:
            S[s]["month1"], S[s]["month2"], S[s]["month_wt1"] = 0, 1, 0.9 - 0.01 * s
        S[s]["month_wt2"] = 1.0 - S[s]["month_wt1"]
    return S


def device(inputs, lib_path=None):
    """A context on the state and geography of _inputs(...) (helpers.device_state)."""
    cols, scal, soil, lat, lon = inputs[:5]
    return H.device_state(cols, scal, soil, lat=lat, lon=lon, lib_path=lib_path)


def _pair(base, graph=True, lib_path=None):
    """Two contexts on the same inputs, the graph on or off in both, at a size whose level stride is padded."""
    A, B = device(base, lib_path), device(base, lib_path)
    A.set_graph(graph)
    B.set_graph(graph)
    assert A.level_stride != A.ncols, f"level stride {A.level_stride} is not padded at {A.ncols} columns"
    return A, B


class StepRows(tuple):
    """What stepwise returns: (conservation [nsteps, 8, 3], flags [nsteps], first [nsteps]) as run_diagnostics gives them, with .bal,
    water_balance's (triples, nbad, first) of every step where RUN_WATER_BALANCE ran, and .qirr, the QFLX_IRRIG row after every step
    where RUN_IRRIGATION ran."""
    bal = qirr = ()


def stepwise(D, rec, steps, flags=0, dt=DT, rec_late=None, late_from=None, rec_times=None, reservoir_time=False, per_step=None):
    """What D.run(dt, steps, flags) does, through the stand-alone calls in RUN_STEP's order (api_run.cpp; launch_advance of elmk_api.cpp
    for the irrigation's place).  This is the one restatement of that order:
      solar geometry; the step's records, uploaded from the host; the record time (rec_times: one per forcing slot); phenology; forcing
      (RUN_QBOT_IS_RH); aerosol deposition (RUN_AEROSOL); init_timestep; water_balance_begin (RUN_WATER_BALANCE); the physics -
      advance_physics or, with RUN_IRRIGATION, its split form: the fused seven, irrigation at the step's time of day (the supply
      limit's launch follows it), soil temperature, snow hydrology, surface fluxes; soil_hydrology (RUN_HYDROLOGY); conservation and
      the flag summary; water_balance (RUN_WATER_BALANCE); the reservoirs' time (reservoir_time: the run derives it from the step, a
      stand-alone call is told) then routing (RUN_ROUTING); active_layer_update with the step's rollover bits (RUN_ALT); accum_update
      (RUN_ACCUM); history_accumulate (RUN_HISTORY).
    rec_late: the records from step late_from on.  per_step: (list, function) - the list receives function(D) after every step."""
    on = lambda f: bool(flags & f)  # noqa: E731
    cons, fo, fb, bal, qirr = [], [], [], [], []
    for s, p in enumerate(steps):
        R = rec_late if (rec_late is not None and s >= late_from) else rec
        decday, doy = float(p["decday"]), int(p["doy"])
        D.solar_geometry(dt, decday, doy)
        f = int(p["forc_slot"])
        for k in st.SERIES_FORCING:
            D.upload(k, np.stack([R[k][f], R[k][f + 1]], axis=1))
        for k in st.SERIES_PHENOLOGY:
            D.upload(k, np.stack([R[k][p["month1"]], R[k][p["month2"]]], axis=1))
        if rec_times is not None:
            D.set_forcing_record_time(rec_times[f])
        st.compute_phenology(D, float(p["month_wt1"]), float(p["month_wt2"]))
        st.get_forcing(D, p["forc_wt1"], p["forc_wt2"], on(st.RUN_QBOT_IS_RH))
        if on(st.RUN_AEROSOL):
            D.aerosol_deposition(int(p["month1"]), int(p["month2"]), float(p["month_wt1"]), float(p["month_wt2"]))
        st.kokkos_init_timestep(D)
        if on(st.RUN_WATER_BALANCE):
            D.water_balance_begin()
        if on(st.RUN_IRRIGATION):
            st.timestep7_fused(D, dt)
            D.irrigation(dt, ir.time_of_day(decday, doy))
            st.kokkos_soil_temperature(D, dt)
            st.kokkos_snow_hydrology(D, dt)
            st.kokkos_surface_fluxes(D, dt)
        else:
            st.advance_physics(D, dt)
        if on(st.RUN_HYDROLOGY):
            D.soil_hydrology(dt)
        cons.append(st.kokkos_evaluate_conservation(D, dt))
        flagged, first = D.error_summary()
        fo.append(flagged)
        fb.append(first)
        if on(st.RUN_WATER_BALANCE):
            bal.append(D.water_balance(dt))
        if on(st.RUN_IRRIGATION):
            qirr.append(D.irrigation_read(ir.QFLX_IRRIG))
        if on(st.RUN_ROUTING):
            if reservoir_time:
                D.routing_reservoir_time(rt.month_of_doy(doy), rt.month_begins(doy, decday))
            D.routing(dt)
        if on(st.RUN_ALT):
            D.active_layer_update(al.rollover(doy, decday))
        if on(st.RUN_ACCUM):
            D.accum_update()
        if on(st.RUN_HISTORY):
            D.history_accumulate()
        if per_step is not None:
            per_step[0].append(per_step[1](D))
    out = StepRows((np.array(cons), np.array(fo, np.uint32), np.array(fb, np.int64)))
    out.bal, out.qirr = bal, qirr
    return out


def upload_series(D, rec, forc_slots=None):
    for k in st.SERIES_FORCING:
        sl = range(rec[k].shape[0]) if forc_slots is None else forc_slots
        D.series_upload(k, sl[0], rec[k][sl[0]:sl[-1] + 1])
    for k in st.SERIES_PHENOLOGY:
        D.series_upload(k, 0, rec[k])


def demo_records(lat, lon, rec):
    """The records that the examples driven by elmk_run read after the state (support.state_blob): geography and the series."""
    return [("lat", lat), ("lon", lon)] + [(f"series/{k}", np.ascontiguousarray(rec[k], np.float64)) for k in SERIES]


def poison(D):
    """Every field a restart image does not hold: NaN, or an out-of-the-way integer."""
    for name, (fid, nlev, dt) in D.fields.items():
        if st.field_class(name) not in IMAGE_CLASSES:
            D.fill(name, np.nan if dt == np.float64 else 3.0)


def assert_same_state(A, B, cols):
    """Every field but the series inputs bit for bit; the series inputs of the run context (B) untouched."""
    for name in A.fields:
        if name in SERIES:
            assert same(B[name], np.ascontiguousarray(cols[name], dtype=B[name].dtype)), f"series input {name} of the run context against the upload"
        else:
            assert same(A[name], B[name]), f"field {name} of the stepwise context against the run context"


def snapshot(D, **rows):
    """Every non-series field and, under each keyword, the rows the caller read beside them."""
    out = {k: D[k] for k in D.fields if k not in SERIES}
    out.update(rows)
    return out


def assert_same(a, b, skip=()):
    """Two snapshots bit for bit, key by key."""
    assert a.keys() == b.keys()
    for k, v in a.items():
        assert k in skip or same(v, b[k]), k


def assert_same_rows(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), f"diagnostics row set {i} (0 conservation, 1 flags, 2 first column): got against want"


# ---- history tapes on the host ------------------------------------------------------------------------------------------------------
class NumpyTapes:
    """The contract of include/elmk.h applied on the host: fp64 accumulators, one fold per sample in step order."""

    INIT = {"avg": -0.0, "sum": -0.0, "max": -np.inf, "min": np.inf, "inst": np.nan}

    def __init__(self, entries):
        self.entries = entries
        self.acc = [None] * len(entries)
        self.count = [0] * st.HIST_MAX_TAPES

    def reset(self, tape):
        self.count[tape] = 0
        for k, (t, _, _) in enumerate(self.entries):
            if t == tape:
                self.acc[k] = None

    def fold(self, values):
        for k, (t, name, op) in enumerate(self.entries):
            v = values[name].astype(np.float64)
            a = self.acc[k] if self.acc[k] is not None else np.full(v.shape, self.INIT[op])
            if op in ("avg", "sum"):
                a = a + v
            elif op == "max":
                a = np.where((v > a) | (v != v), v, a)
            elif op == "min":
                a = np.where((v < a) | (v != v), v, a)
            else:
                a = v.copy()
            self.acc[k] = a
        for t in {t for t, _, _ in self.entries}:
            self.count[t] += 1

    def result(self, k):
        t, _, op = self.entries[k]
        return self.acc[k] / float(self.count[t]) if op == "avg" else self.acc[k]


# ---- one step under per-column solar geometry, on the device and in the oracle group by group ------------------------------------------
FORC_WT = np.random.default_rng(3).random(8)


def _global_pair(n, seed, lat=None, lon=None, tier="B"):
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier=tier, seed=seed)
    if lat is None:
        lat, lon = synth.global_grid(n, seed=seed)
    return H.device_state(cols, scal, soil, lat=lat, lon=lon), cols, scal, soil


def _groups(dayl, max_dayl):
    key = np.stack([dayl.view(np.uint64), max_dayl.view(np.uint64)], axis=1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    return [(uniq[g, 0:1].view(np.float64)[0], uniq[g, 1:2].view(np.float64)[0], inv.reshape(-1) == g) for g in range(len(uniq))]


def _oracle_step(S, coszen):
    S["coszen"][...] = coszen.reshape(S["coszen"].shape)
    S.phenology(0.3, 0.7)
    S.get_forcing(1.0 - FORC_WT, FORC_WT, False)
    S.init_timestep()
    S.timestep7(DT)
    S.soil_temperature(DT)
    S.snow_hydrology(DT)
    S.surface_fluxes(DT)


def _device_step(D, how):
    st.compute_phenology(D, 0.3, 0.7)
    st.get_forcing(D, 1.0 - FORC_WT, FORC_WT, False)
    st.kokkos_init_timestep(D)
    if how == "advance":
        st.advance_physics(D, DT)
    else:
        (st.timestep7_fused if how == "fused" else st.timestep7)(D, DT)
        st.kokkos_soil_temperature(D, DT)
        st.kokkos_snow_hydrology(D, DT)
        st.kokkos_surface_fluxes(D, DT)
