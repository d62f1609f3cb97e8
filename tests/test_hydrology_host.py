"""Soil hydrology on the host (include/elmk.h "soil hydrology"; elmkernels_amd/hydrology.py): hand-checked columns of `step`, the exact
water budget of one step, the parameter helpers, the header's constants and symbols, and restart images of version 4; and the
generators of the stage's inputs: `generated` (every branch) and `edge_columns` (the edge tier; tests/test_hydrology_edges_host.py)."""
import math
import os
import re

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import hydrology as hy
from elmkernels_amd import restart as R
from elmkernels_amd import state as st
from elmkernels_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1800.0
N = hy.N
BRANCHES = {"jwt_0", "jwt_mid", "jwt_N", "infiltration_excess", "h2osfc_above_threshold", "h2osfc_below_threshold", "h2osfc_runoff",
            "h2osfc_negative", "imped", "table_rises", "table_falls", "drain_aquifer", "drain_soil", "excess_up", "excess_to_h2osfc",
            "watmin_push_down", "watmin_search", "watmin_remainder", "snl_0", "snl_pos"}


def prepare(cols, seed, sfc_every=4):
    """The branch-mix generator's columns (synth.make_state) with the rows the stage reads set so that every branch of it occurs:
    rain up to infiltration excess, root uptake, ice in the top three layers, near-saturated and near-dry layers, h2osfc above and below
    its threshold (in two of every sfc_every columns), and water tables from the top layer down to 12 m.  Changes cols in place; returns the rows of the feature [NROWS, n]."""
    n = cols["snl"].shape[0]
    rng = np.random.default_rng(seed)
    c = np.arange(n)
    s0, s1 = hy.NLEVSNO, hy.NLEVSNO + N
    dzmm = cols["dz"][:, s0:s1] * 1.0e3
    watsat = cols["watsat"][:, :N]
    top = rng.uniform(0.0, 3.0e-4, n)
    top[c % 6 == 0] = 0.0
    top[c % 6 == 1] = rng.uniform(0.02, 0.08, (c % 6 == 1).sum())  # heavier than any hksat: infiltration excess
    cols["qflx_top_soil"] = top
    root = np.zeros((n, 15))
    root[:, :8] = rng.uniform(0.0, 2.0e-6, (n, 8))
    cols["qflx_rootsoi"] = root
    liq, ice = cols["h2osoi_liq"], cols["h2osoi_ice"]
    m = c % 5 == 1  # ice in the top three layers
    ice[m, s0:s0 + 3] = (rng.uniform(0.2, 1.1, (m.sum(), 3)) * watsat[m, :3]) * dzmm[m, :3] * 0.917
    m = c % 7 == 2  # near-saturated
    liq[m, s0:s1] = np.maximum(0.995 * watsat[m] * dzmm[m] - ice[m, s0:s1], 0.02)
    m = c % 7 == 3  # near-dry, below watmin in places
    liq[m, s0:s1] = rng.choice([0.002, 0.008, 0.05, 0.5], (m.sum(), N))
    m = c % 21 == 10  # the bottom layer below watmin over layers that can spare water
    liq[m, s1 - 1] = 0.001
    hs = np.zeros(n)
    fh = np.zeros(n)
    k = sfc_every
    hs[c % k == 0], fh[c % k == 0] = 20.0 + rng.random((c % k == 0).sum()), 0.6
    hs[c % k == 1], fh[c % k == 1] = 0.5, 0.2
    cols["h2osfc"], cols["frac_h2osfc"] = hs, fh
    ev = cols["qflx_ev_h2osfc"]
    ev[c % (2 * k) == k + 1] = 1.0e-2  # evaporation beyond the store: h2osfc would go negative
    rows = np.zeros((hy.NROWS, n))
    zw = np.array([0.01, 0.05, 0.3, 1.0, 2.5, 3.7, 3.9, 8.8, 12.0])
    rows[hy.ZWT] = zw[c % zw.size] * (1.0 + 0.05 * rng.random(n))
    rows[hy.WA] = np.where(c % 11 == 0, 4999.9999, 4000.0 + 100.0 * rng.random(n))
    sand, clay = rng.uniform(5.0, 90.0, (n, N)), rng.uniform(2.0, 50.0, (n, N))
    om = np.where(rng.random((n, N)) < 0.3, rng.uniform(60.0, 130.0, (n, N)), rng.uniform(0.0, 30.0, (n, N)))
    rows[hy.HKSAT:hy.HKSAT + N] = hy.hksat_from_texture(sand, clay, om, cols["zsoi"][:, s0:s1])
    slope = rng.uniform(0.0, 12.0, n)
    rows[hy.WTFACT] = rng.uniform(0.05, 0.6, n)
    rows[hy.H2OSFC_THRESH] = hy.h2osfc_thresh(rng.uniform(0.005, 0.05, n))
    rows[hy.K_WET] = hy.k_wet(slope)
    rows[hy.RSUB_TOP_MAX] = hy.rsub_top_max(slope)
    return rows


def clear_snow(cols, every=8):
    """Make all but one column in `every` snow-free and keep them so (no snowfall): the generator's snow share plus the columns
    that pond would otherwise leave under half of the columns to the closure."""
    m = np.arange(cols["snl"].shape[0]) % every != every - 1
    for k in ("h2osno", "snow_depth", "frac_sno", "frac_sno_eff", "int_snow", "forc_snow"):
        cols[k][m] = 0.0
    cols["snl"][m] = 0
    for k in ("h2osoi_liq", "h2osoi_ice", "dz", "zsoi", "zisoi"):
        cols[k][m, :hy.NLEVSNO] = 0.0


def generated(n, seed, sfc_every=4, full=False, chain=False):
    cols, scal, soil = synth.make_state(st.field_table(), n, tier="B", seed=seed)
    if chain:
        sfc_every = CHAIN_SFC_EVERY
        clear_snow(cols)
    rows = prepare(cols, seed + 1, sfc_every)
    return (cols, scal, soil, rows) if full else (cols, rows)


# ---- the edge tier ------------------------------------------------------------------------------------------------------------------
SOIL_FIELDS = ("h2osoi_liq", "h2osoi_ice", "dz", "zsoi", "zisoi")  # fields that carry the snow levels: layer j is level NLEVSNO + j
POISONS = (float("nan"), float("inf"), float("-inf"))
POISONED_ROWS = tuple(range(hy.ZWT, hy.RSUB_TOP_MAX + 1))  # ZWT, WA, the ten HKSAT rows, WTFACT .. RSUB_TOP_MAX
# snl is the one integer field of hydrology.READS: it has no NaN and no infinity
POISONED_FIELDS = tuple(k for k in hy.READS if k != "snl") + ("t_soisno",)


def edge_classes():
    """The classes of edge_columns in the order they are dealt: [(name, function of (E, i, k))], E the _Edge under construction, i the
    column and k a counter that moves the layer a class touches from one round of the classes to the next."""
    s0 = hy.NLEVSNO
    out = []
    turn = (9, 0, 5, 1, 8, 2, 7, 3, 6, 4)  # the layer of round k: the bottom and the top layer first

    def add(name):
        def deco(f):
            out.append((name, f))
            return f
        return deco

    def dzmm(E, i, j):
        return float(E.cols["dz"][i, s0 + j]) * 1.0e3

    def wet(E, i, hs=20.0, fh=0.6):
        E.cols["h2osfc"][i], E.cols["frac_h2osfc"][i] = hs, fh

    # the water table and the aquifer
    add("zwt=0")(lambda E, i, k: E.row(hy.ZWT, i, 0.0))
    add("zwt=1e-9")(lambda E, i, k: E.row(hy.ZWT, i, 1.0e-9))
    for j in range(N):
        @add(f"zwt=zisoi[{j}]")
        def _(E, i, k, j=j):
            # (the interfaces of this column are made fp32 values, so that the equality holds in the fp32-state build too)
            E.cols["zisoi"][i] = E.cols["zisoi"][i].astype(np.float32)
            E.row(hy.ZWT, i, float(E.cols["zisoi"][i, s0 + j + 1]))
    add("zwt=80")(lambda E, i, k: E.row(hy.ZWT, i, 80.0))
    add("zwt=100")(lambda E, i, k: E.row(hy.ZWT, i, 100.0))
    add("zwt just below the column")(lambda E, i, k: E.row(hy.ZWT, i, float(np.nextafter(E.cols["zisoi"][i, s0 + N], 100.0))))
    add("wa=0")(lambda E, i, k: E.row(hy.WA, i, 0.0))

    @add("wa=0, table below")
    def _(E, i, k):
        E.row(hy.WA, i, 0.0)
        E.row(hy.ZWT, i, 8.0)

    @add("wa=5000")
    def _(E, i, k):
        E.row(hy.WA, i, 5000.0)
        E.row(hy.ZWT, i, 8.0)

    @add("wa>5000")
    def _(E, i, k):
        E.row(hy.WA, i, 5500.0)
        E.row(hy.ZWT, i, 8.0)
        E.row(hy.RSUB_TOP_MAX, i, 0.0)

    # conductivity, ice and water content
    add("hksat=0 in one layer")(lambda E, i, k: E.row(hy.HKSAT + k % N, i, 0.0))

    @add("hksat=0")
    def _(E, i, k):
        E.rows[hy.HKSAT:hy.HKSAT + N, i] = 0.0
    add("rsub_top_max=0")(lambda E, i, k: E.row(hy.RSUB_TOP_MAX, i, 0.0))

    @add("ice beyond the pores")
    def _(E, i, k):
        for j in range(k % 4, N, 3):
            E.cols["h2osoi_ice"][i, s0 + j] = 1.5 * float(E.cols["watsat"][i, j]) * dzmm(E, i, j) * 0.917

    @add("liq=0 in one layer")
    def _(E, i, k):
        E.cols["h2osoi_liq"][i, s0 + k % N] = 0.0

    @add("liq=0")
    def _(E, i, k):
        E.cols["h2osoi_liq"][i, s0:s0 + N] = 0.0

    @add("liq<1e-6")
    def _(E, i, k):
        E.cols["h2osoi_liq"][i, s0:s0 + N] = 9.0e-8 * (1.0 + np.arange(N))

    @add("bottom layer under 1 %, table below")
    def _(E, i, k):
        E.cols["h2osoi_liq"][i, s0 + N - 1] = 0.004 * float(E.cols["watsat"][i, N - 1]) * dzmm(E, i, N - 1)
        E.cols["h2osoi_ice"][i, s0 + N - 1] = 0.0
        E.row(hy.ZWT, i, 8.0)

    @add("table layer under 1 %")
    def _(E, i, k):
        j = 2 + k % 7
        E.cols["h2osoi_liq"][i, s0 + j] = 0.004 * float(E.cols["watsat"][i, j]) * dzmm(E, i, j)
        E.cols["h2osoi_ice"][i, s0 + j] = 0.0
        E.row(hy.ZWT, i, float(E.cols["zsoi"][i, s0 + j]))

    @add("root uptake beyond the water")
    def _(E, i, k):
        j = k % 8
        E.cols["qflx_rootsoi"][i, j] = 2.0 * float(E.cols["h2osoi_liq"][i, s0 + j])

    # the surface fractions
    add("frac_h2osfc=0")(lambda E, i, k: wet(E, i, 0.0, 0.0))
    add("frac_h2osfc=0.4")(lambda E, i, k: wet(E, i, 20.0, 0.4))
    add("frac_h2osfc=1")(lambda E, i, k: wet(E, i, 30.0, 1.0))
    add("frac_h2osfc just above 0.4")(lambda E, i, k: wet(E, i, 20.0, float(np.nextafter(0.4, 1.0))))

    @add("h2osfc at its threshold")
    def _(E, i, k):
        wet(E, i, float(E.rows[hy.H2OSFC_THRESH, i]))

    @add("no rain, evaporation")
    def _(E, i, k):
        E.cols["qflx_top_soil"][i] = 0.0
        E.cols["qflx_evap_grnd"][i] = E.cols["qflx_ev_soil"][i] = 1.0e-4

    @add("frac_sno_eff=0")
    def _(E, i, k):
        E.cols["frac_sno_eff"][i] = 0.0

    @add("frac_sno_eff=1")
    def _(E, i, k):
        E.cols["frac_sno_eff"][i] = 1.0

    @add("tiny k_wet")
    def _(E, i, k):
        wet(E, i)
        E.row(hy.K_WET, i, 1.0e-6)

    # the soil parameters
    def params(name, bsw=None, sucsat=None, watsat=None, also=None):
        @add(name)
        def _(E, i, k):
            for key, v in (("bsw", bsw), ("sucsat", sucsat), ("watsat", watsat)):
                if v is not None:
                    E.cols[key][i, :N] = v
            if also:
                also(E, i, k)

    def dry(E, i, k):
        E.cols["h2osoi_liq"][i, s0:s0 + N] = 0.02
        E.cols["h2osoi_ice"][i, s0:s0 + N] = 0.0

    def deep(E, i, k):
        E.row(hy.ZWT, i, 80.0)
    params("bsw=1.5", bsw=1.5)
    params("bsw=20", bsw=20.0)
    params("sucsat=10", sucsat=10.0)
    params("sucsat=1000", sucsat=1000.0)
    params("watsat=0.2", watsat=0.2)
    params("watsat=0.9", watsat=0.9)
    params("bsw=20, sucsat=1000, dry", bsw=20.0, sucsat=1000.0, also=dry)       # smp at SMPMIN
    params("bsw=1.5, sucsat=10, deep table", bsw=1.5, sucsat=10.0, also=deep)  # the equilibrium profile under 1 % of saturation
    params("layered parameters", bsw=np.array([1.5, 20.0, 3.0, 12.0, 1.5, 20.0, 7.0, 2.0, 16.0, 5.0]),
           sucsat=np.array([10.0, 1000.0, 40.0, 600.0, 1000.0, 10.0, 200.0, 90.0, 15.0, 800.0]),
           watsat=np.array([0.9, 0.2, 0.6, 0.3, 0.2, 0.9, 0.45, 0.8, 0.25, 0.5]))

    # the walks: over a wet column a shallow table rises through the layers; a strong drainage runs down through them
    @add("rise to the surface")
    def _(E, i, k):
        E.cols["h2osoi_ice"][i, s0:s0 + N] = 0.0
        for j in range(N):
            E.cols["h2osoi_liq"][i, s0 + j] = 0.999 * float(E.cols["watsat"][i, j]) * dzmm(E, i, j)
        E.rows[hy.HKSAT:hy.HKSAT + N, i] = 0.5
        # a small specific yield: the recharge, bounded by 10 mm a step, fills layer after layer
        E.cols["bsw"][i, :N], E.cols["sucsat"][i, :N] = 20.0, 1000.0
        E.row(hy.ZWT, i, float(E.cols["zsoi"][i, s0 + 2 + k % 4]))

    @add("drain through the column")
    def _(E, i, k):
        E.row(hy.RSUB_TOP_MAX, i, 50.0 if k % 2 else 0.05)
        E.row(hy.ZWT, i, float(E.cols["zsoi"][i, s0 + 1 + k % 4]))

    @add("fall through the column")
    def _(E, i, k):
        # drier than the equilibrium over a shallow table: the recharge is negative and at its bound
        E.cols["h2osoi_ice"][i, s0:s0 + N] = 0.0
        for j in range(N):
            E.cols["h2osoi_liq"][i, s0 + j] = 0.3 * float(E.cols["watsat"][i, j]) * dzmm(E, i, j)
        E.rows[hy.HKSAT:hy.HKSAT + N, i] = 5.0
        E.cols["bsw"][i, :N] = 1.5
        E.row(hy.ZWT, i, float(E.cols["zsoi"][i, s0 + (6 if k % 2 else 1)]))

    # the frost form
    @add("t_soisno=tfrz at the front")
    def _(E, i, k):
        kf = 1 + k % (N - 1)
        E.cols["t_soisno"][i, s0:s0 + kf] = 275.0
        E.cols["t_soisno"][i, s0 + kf:s0 + N] = hy.TFRZ

    @add("q_perch_max=0")
    def _(E, i, k):
        if E.frost is not None:
            E.frost[hy.Q_PERCH_MAX, i] = 0.0

    @add("dz=0 in one layer")
    def _(E, i, k):
        E.cols["dz"][i, s0 + turn[k % N]] = 0.0

    # the non-finite tier: one poisoned input per column
    for v in POISONS:
        for key in POISONED_FIELDS:
            @add(f"{key}={v}")
            def _(E, i, k, key=key, v=v):
                a = E.cols[key]
                if a.ndim == 1:
                    a[i] = v
                elif key in SOIL_FIELDS or key == "t_soisno":
                    a[i, s0 + turn[k % N]] = v
                else:
                    a[i, turn[k % N]] = v
        for w in POISONED_ROWS:
            add(f"row {w}={v}")(lambda E, i, k, w=w, v=v: E.row(w, i, v))

        @add(f"q_perch_max={v}")
        def _(E, i, k, v=v):
            if E.frost is not None:
                E.frost[hy.Q_PERCH_MAX, i] = v

        # the aquifer node takes the bottom layer's parameters: poisoned under a table below the column
        for key in ("watsat", "sucsat", "bsw"):
            @add(f"table below, bottom {key}={v}")
            def _(E, i, k, key=key, v=v):
                E.cols[key][i, N - 1] = v
                E.row(hy.ZWT, i, 8.0)
    return out


class _Edge:
    def __init__(self, cols, rows, frost):
        self.cols, self.rows, self.frost = cols, rows, frost

    def row(self, w, i, v):
        self.rows[w, i] = v


EDGE_CLASS_NAMES = tuple(name for name, _ in edge_classes())


def edge_class_of(n):
    """The class of every column of edge_columns(n, ...): an index into EDGE_CLASS_NAMES."""
    return np.arange(n) % len(EDGE_CLASS_NAMES)


def edge_finite(n):
    """The columns of edge_columns(n, ...) outside the non-finite tier."""
    first = EDGE_CLASS_NAMES.index("dz=0 in one layer")
    return edge_class_of(n) < first


def edge_columns(n, seed, frost=False, full=False, skip=()):
    """The edge tier of the stage: generated (frost: generated_frost) with one edge per column, the classes of edge_classes() dealt to
    the columns in turn and the layer a class touches moved on with every round.  A class changes only what it names, so every edge
    meets the generator's mix of the other inputs.  skip: names of classes left as the generator made them (the census test shows
    with it that a class is needed).  Returns (cols, [scal, soil,] rows[, frost rows])."""
    cols, scal, soil, rows = generated(n, seed, full=True)
    fr = None
    if frost:
        from tests.test_frost_table_host import add_frost

        fr = add_frost(cols, rows, seed + 2)
    for k in POISONED_FIELDS + ("qflx_rootsoi",):
        cols[k] = np.array(cols[k], dtype=np.float64)
    E = _Edge(cols, rows, fr)
    classes = edge_classes()
    assert not set(skip) - set(EDGE_CLASS_NAMES)
    for i in range(n):
        name, f = classes[i % len(classes)]
        if name not in skip:
            f(E, i, i // len(classes))
    out = (cols, scal, soil, rows) if full else (cols, rows)
    return out + (fr,) if frost else out


# ---- the chain: the physics of one step, then the stage -----------------------------------------------------------------------------
CHAIN_STEPS = 6
CHAIN_SFC_EVERY = 16  # surface water in one column of eight: with the snow columns, under half are left out of the closure
# |errh2o| of the closed budget over the snow-free columns without surface water of the six-step host chain of
# generated(1001, 77, chain=True): the largest value measured on the host (mm; its median there is 3.3e-13).  The maximum comes from
# a few columns where the reference's snow hydrology sets the ice of the top soil layer to the literal 0.9 when sublimation would
# take it below zero (src/physics/snow_hydrology_impl.hh:303 and :311, `h2osoi_ice(top) = 0.9` with top = the first soil layer for
# snl == 0): 0.9 mm that no flux accounts for.  The bound is ten times the maximum, headroom over one seed; at 9 mm it lies far above
# the budget without the stage (median 1.9e-2 mm) and can only catch a gross fault - the bit equality with the host chain and the
# medians carry the closure tests.
CLOSURE_MEASURED = 0.9000328415202219
CLOSURE_BOUND = 10.0 * CLOSURE_MEASURED


def water_mass(f):
    """column_water_mass in the conservation kernel's order: h2ocan + h2osno + h2osfc, then ice + liq of the 20 levels in turn."""
    w = (f["h2ocan"].astype(np.float64) + f["h2osno"].astype(np.float64)) + f["h2osfc"].astype(np.float64)
    for i in range(20):
        w = w + (f["h2osoi_ice"][:, i].astype(np.float64) + f["h2osoi_liq"][:, i].astype(np.float64))
    return w


CLOSURE_FIELDS = ("h2ocan", "h2osno", "h2osfc", "h2osoi_ice", "h2osoi_liq", "dtbegin_column_h2o", "forc_rain", "forc_snow", "qflx_evap_tot",
                  "qflx_snwcp_ice", "snl", "frac_h2osfc")


def closure(f, wa_beg, h2osno_beg, rows_out, dt, with_stage=True):
    """(errh2o per column, the columns it is judged on) from the fields after a step: hydrology.water_balance_error with the stage's
    runoff and drainage (or, with_stage False, the reference's hardwired zero and no aquifer); snow-free columns (no snow mass before or after the step: the reference's snow hydrology drops a layerless snow cover
    without a flux) without surface water."""
    z = np.zeros(wa_beg.shape)
    e = hy.water_balance_error(f["dtbegin_column_h2o"], water_mass(f), wa_beg, rows_out[hy.WA] if with_stage else wa_beg, f["forc_rain"],
                               f["forc_snow"], f["qflx_evap_tot"], f["qflx_snwcp_ice"], *((rows_out[hy.QFLX_SURF], rows_out[hy.QFLX_H2OSFC_SURF],
                                                                                         rows_out[hy.QFLX_DRAIN]) if with_stage else (z, z, z)), dt)
    keep = (f["snl"] == 0) & (f["h2osno"] == 0.0) & (h2osno_beg == 0.0) & (f["frac_h2osfc"] == 0.0)
    return e, keep


def host_chain(cols, scal, soil, rows, nsteps=CHAIN_STEPS, dt=DT, stage=True):
    """The oracle's step (init_timestep, the seven wrappers, soil temperature, snow hydrology, surface fluxes) and then hydrology.step,
    nsteps times.  Returns the oracle state, the rows, and per step (errh2o, keep) of closure()."""
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
        if stage:
            out, rows = hy.step(S.fields, rows, dt)
            for k, v in out.items():
                S.fields[k][...] = v
        per_step.append(closure({k: np.array(S.fields[k]) for k in CLOSURE_FIELDS}, wa_beg, h2osno_beg, rows, dt, stage))
    return S, rows, per_step


# ---- hand-built columns -----------------------------------------------------------------------------------------------------------
def column(zwt=1.0, wa=4000.0, hksat=0.0, sat=0.5, **kw):
    """A uniform loam column on ELM's grid: watsat 0.45, sucsat 200 mm, bsw 5; liq = sat * watsat * dzmm; no ice, no fluxes, no
    runoff parameters.  Keywords replace entries."""
    zi = [0.0, 0.0175, 0.0451, 0.0906, 0.1655, 0.2891, 0.4929, 0.8289, 1.3828, 2.2961, 3.8019]
    dz = [zi[j + 1] - zi[j] for j in range(N)]
    z = [0.5 * (zi[j + 1] + zi[j]) for j in range(N)]
    c = {"liq": [sat * (0.45 * (d * 1.0e3)) for d in dz], "ice": [0.0] * N, "dz": dz, "z": z, "zi": zi, "watsat": [0.45] * N,
         "sucsat": [200.0] * N, "bsw": [5.0] * N, "rootsoi": [0.0] * N, "hksat": [hksat] * N, "snl": 0, "fsno": 0.0, "h2osfc": 0.0,
         "frac_h2osfc": 0.0, "qflx_top_soil": 0.0, "qflx_evap_grnd": 0.0, "qflx_ev_soil": 0.0, "qflx_ev_h2osfc": 0.0, "qflx_dew_grnd": 0.0,
         "qflx_dew_snow": 0.0, "qflx_sub_snow": 0.0, "zwt": zwt, "wa": wa, "wtfact": 0.0, "h2osfc_thresh": 5.0, "k_wet": 0.05,
         "rsub_top_max": 0.0}
    c.update(kw)
    return c


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
