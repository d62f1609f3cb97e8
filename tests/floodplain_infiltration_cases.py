"""The inputs of the floodplain infiltration's tests, host and device (include/elmk.h "floodplain infiltration"): the three map shapes
with every column in at most one cell, the columns (the soil hydrology's generated tier with every fifth column draining a thousand
times faster, so that the floodplain's depth and not qinmax limits the drain there), the cells (the inundation's cell values, with the
edge values of WF in cells of their own and the cells the census needs), F0 restated, the census of F1's branches, one step of the
three stages on the host, and the closed systems of the budget tests."""
import numpy as np

from elmkernels_amd import hydrology as hy
from elmkernels_amd import regrid
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import inundation_cases as ic
from tests.hydrology_cases import add_frost, clear_snow, prepare, water_mass

DT = 1800.0
NSUB = 3
NSTEPS = 5
NAN, INF = float("nan"), float("inf")
SHAPES = ("one", "wide", "single")
# F1's branches as the census names them: the operand the guard fails on first, or the side of the minimum
BRANCHES = ("no cell", "WF fails", "FLOOD_FRAC fails", "a < b", "a >= b")
BIG_CELL, NO_AREA_CELL, NAN_QINMAX_CELL = 40, 18, 42  # of the wide and the single shape
NO_FLOODPLAIN_CELLS = tuple(range(24, 40, 2)) + tuple(range(46, 60))  # cells no wider than their channel: AF = 0


# ---- maps ------------------------------------------------------------------------------------------------------------------------------
def cell_map(shape, seed=5, partition=False):
    """(ncols, ncells, ptr, col, w) with every column in at most one cell.
      "one":    1 column in 1 cell.
      "wide":   5003 columns over 70 cells: cell 40 has 2100 columns (past a workgroup and past an LDS tile of the map walkers), cells 0
                and 60 .. 67 have none (empty cells across the 64-cell boundary), 300 columns are in no cell, every other cell has at
                least one.
      "single": 1001 cells of one column each, and 9 more columns in no cell.
      "run":    300 columns, 65 cells of 0 .. 4 columns each.
    The columns are dealt in a random order.  Weights: per term u / (the cell's terms), u in 0.3 .. 1, so that a cell's weights sum to
    at most one and a floodplain outlives a step in which its columns take all they can; partition: exactly 1 / (the cell's terms)."""
    rng = np.random.default_rng(seed)
    if shape == "one":
        ncols, cnt, free = 1, np.array([1]), 0
    elif shape == "wide":
        ncols, free = 5003, 300
        cnt = np.ones(70, np.int64)
        cnt[[0] + list(range(60, 68))] = 0
        cnt[BIG_CELL] = 2100
        rest = ncols - free - int(cnt.sum())
        others = np.nonzero((cnt == 1))[0]
        cnt[others] += rng.multinomial(rest, np.full(others.size, 1.0 / others.size))
    elif shape == "single":
        ncols, cnt, free = 1010, np.ones(1001, np.int64), 9
    elif shape == "run":  # the run tests': 300 columns, 65 cells (one past the 64-cell padding) of 0 .. 4 columns
        ncols = 300
        cnt = rng.integers(0, 5, 65)
        free = ncols - int(cnt.sum())
    else:
        raise ValueError(shape)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = rng.permutation(ncols)[free:].astype(np.int32)
    assert col.size == ptr[-1]
    per = np.repeat(cnt, cnt).astype(np.float64)
    w = (1.0 if partition else rng.uniform(0.3, 1.0, col.size)) / per
    return ncols, cnt.size, ptr, col, np.ascontiguousarray(w, dtype=np.float64)


def cellof(ncols, ptr, col):
    """F0: the cell whose CSR span names column c, -1 for a column in no cell; int32 [ncols].  Raises ValueError with the entry point's
    words for the first column (in term order) that an earlier term holds already."""
    out = np.full(ncols, -1, np.int32)
    seen = np.zeros(ncols, bool)
    for c in np.asarray(col).tolist():
        if c < 0 or c >= ncols:
            raise IndexError("col outside [0, ncols)")
        if seen[c]:
            raise ValueError(f"column {c} is in more than one cell of the output grid (or twice in one)")
        seen[c] = True
    for g in range(len(ptr) - 1):
        out[col[ptr[g]:ptr[g + 1]]] = g
    return out


# ---- columns and cells -----------------------------------------------------------------------------------------------------------------
def columns(ncols, seed, frost=False):
    """(cols, scal, soil, rows, frost rows or None): the soil hydrology's generated tier, snow cleared; columns 2, 7, 12 .. conduct a
    thousand times better, so that there a = FLOOD_FRAC qinmax lies above b = H2OROF / dt."""
    cols, scal, soil = synth.make_state(st.field_table(), ncols, tier="B", seed=seed)
    clear_snow(cols)
    rows = prepare(cols, seed + 1)
    rows[hy.HKSAT:hy.HKSAT + hy.N, 2::5] *= 1000.0
    fr = add_frost(cols, rows, seed + 2) if frost else None
    return cols, scal, soil, rows, fr


def finite(x, fill=7.0):
    return np.where(np.isfinite(x) & (np.abs(x) < 1e200), x, fill)


def cells(ncells, seed, nsub=NSUB, dt=DT):
    """A dict of the cells' values: down, ddist, area, p, rdepth, eprof, and the initial volr, wh, wt, wf.  The inundation's cell values
    (inundation_cases.flood_values: the placed cells stand flooded through the chain; cells 2, 4 .. 16 hold the edge values of WF -
    zero, negative zero, negative, denormal, 1e300, NaN, +inf, -inf) with the storages of the river made finite; cell 18 (no area)
    and the cells NO_FLOODPLAIN_CELLS (no wider than their channel, so AF = 0) stand over their banks: all their water stands in the channel's
    prism, FLOOD_FRAC is zero, and WF is what the rounding of W - vc2 leaves, zero or a few units in the last place above it - the one
    way a wet floodplain meets a FLOOD_FRAC of zero after a routing call; cell 42 is an outlet: the column with a NaN
    qinmax drains into it and its NaN goes no further."""
    ddist, area, p, volr, wh, wt = ic.cell_values(ncells, seed)
    volr, wh, wt = finite(volr), finite(wh), finite(wt)
    rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(ncells, seed + 1, area, p, volr, wh, wt, nsub, dt)
    down = ic.networks(ncells, seed + 2)["forest"].copy() if ncells >= 3 else np.full(ncells, -1, np.int32)
    if ncells > NAN_QINMAX_CELL:
        vc = (p[rt.RLEN] * p[rt.RWIDTH]) * rdepth
        p[rt.NR, NO_AREA_CELL] = 400.0
        volr[NO_AREA_CELL], wf[NO_AREA_CELL], wh[NO_AREA_CELL], wt[NO_AREA_CELL] = 1.2 * vc[NO_AREA_CELL], 1.0e6, 0.0, 0.0
        down[NAN_QINMAX_CELL] = -1
        for k, c in enumerate(NO_FLOODPLAIN_CELLS + (tuple(range(400, 600)) if ncells >= 600 else ())):  # (and two hundred more where there are cells)
            area[c] = (0.3 + 0.03 * k) * (p[rt.RLEN, c] * p[rt.RWIDTH, c])
            p[rt.NR, c] = 400.0
            volr[c], wf[c], wh[c], wt[c] = (1.1 + 0.037 * k) * vc[c], 1.0e5 * (1 + k), 0.0, 0.0
    else:  # a shape of a few cells: every one of them stands a fifth over its banks under 30 mm of water
        vc = (p[rt.RLEN] * p[rt.RWIDTH]) * rdepth
        p[rt.NR] = 400.0
        volr, wf = 1.2 * vc, 0.03 * area
    return dict(down=down, ddist=ddist, area=area, p=p, rdepth=rdepth, eprof=eprof, volr=volr, wh=wh, wt=wt, wf=wf)


def case(shape, seed, frost=False, partition=False):
    """The whole case of one shape: map, cellof, columns, cells; the column with the NaN qinmax (a NaN WTFACT) is the first column of
    cell 42 where the shape has it."""
    ncols, ncells, ptr, col, w = cell_map(shape, seed, partition)
    cols, scal, soil, rows, fr = columns(ncols, seed + 10, frost)
    G = cells(ncells, seed + 20)
    nanq = -1
    if ncells > NAN_QINMAX_CELL:
        nanq = int(col[ptr[NAN_QINMAX_CELL]])
        rows[hy.WTFACT, nanq] = NAN
    G.update(shape=shape, ncols=ncols, ncells=ncells, map=(ptr, col, w), cellof=cellof(ncols, ptr, col), cols=cols, scal=scal, soil=soil,
             rows=rows, frost=fr, nanq=nanq)
    return G


def run_case(seed=41, frost=False):
    """The case of the run, restart and tape tests: the "run" shape under columns with geography and records (run_cases._inputs), no NaN
    column, the river's edge values made finite."""
    from tests.run_cases import _inputs

    ncols, ncells, ptr, col, w = cell_map("run", seed)
    b = _inputs(ncols, seed + 10)
    clear_snow(b[0])
    rows = prepare(b[0], seed + 11)
    rows[hy.HKSAT:hy.HKSAT + hy.N, 2::5] *= 1000.0
    fr = add_frost(b[0], rows, seed + 12) if frost else None
    G = cells(ncells, seed + 20)
    G["wf"] = finite(G["wf"])
    G.update(shape="run", ncols=ncols, ncells=ncells, map=(ptr, col, w), cellof=cellof(ncols, ptr, col), cols=b[0], scal=b[1], soil=b[2],
             lat=b[3], lon=b[4], rec=b[5], rows=rows, frost=fr, nanq=-1)
    return G


# ---- F1's census -----------------------------------------------------------------------------------------------------------------------
def census(cell_of, wf, ff, fpi):
    """Which branch of F1 every column took, an index into BRANCHES: from the rows the step read (wf, ff over the cells) and wrote
    (fpi [3, ncols]).  (The guard's last operand, area, cannot fail first on the device: a cell of no area has a FLOOD_FRAC of zero, and
    the routing refuses a NaN area.  The host test of the guard meets it.)"""
    g = np.asarray(cell_of)
    safe = np.where(g >= 0, g, 0)
    with np.errstate(all="ignore"):
        w, f = wf[safe], ff[safe]
        passed = (g >= 0) & (w > 0.0) & (f > 0.0)
        b = fpi[hy.FPI_H2OROF] / DT
        return np.where(g < 0, 0, np.where(~(w > 0.0), 1, np.where(~(f > 0.0), 2, np.where(passed & (fpi[hy.FPI_QFLX_DRAIN] == b), 4, 3))))


# ---- one step of the three stages on the host -------------------------------------------------------------------------------------------
STEP_FIELDS = hy.READS + ("h2osoi_vol",)


def host_step(f, rows, wb, river, G, dt=DT, nsub=NSUB, frost=None, qirr=None, dam=None, on=True, stored=None):
    """hydrology.step, water_balance_end and kinematic_call on the fields f (a dict that holds hydrology.READS, h2osoi_vol and
    hydrology.WB_READS; BEGWB is in wb already), the hydrology's rows, the water balance's rows and the river's rows, a dict with wh, wt,
    volr, wf, frac (and res, krls with dam = the reservoirs' tables, month and begins).  on: with the extension.  Returns (fields out,
    rows, frost rows, fpi rows or None, wb, river, qland or None): nothing is changed in place."""
    ptr, col, w = G["map"]
    tab = rt.inundation_tables(G["area"], G["p"], G["rdepth"], G["eprof"])
    up = rt.upstream_map(G["down"])
    rof = (G["cellof"], river["wf"], river["frac"], G["area"]) if on else None
    res = hy.step({k: f[k] for k in STEP_FIELDS + (("t_soisno",) if frost is not None else ())}, rows, dt, frost=frost, rof=rof, stored=stored)
    out, rows_out = res[0], res[1]
    frost_out = res[2] if frost is not None else None
    fpi = res[-1] if on else None
    g = dict(f)
    g.update(out)
    wb = hy.water_balance_end(g, rows_out, wb, dt, frost=frost_out, qflx_irrig=qirr, qflx_h2orof_drain=fpi[hy.FPI_QFLX_DRAIN] if on else None)
    qin = rt.qin_from_rows(ptr, col, w, wb[hy.WB_QRUNOFF], G["area"], qflx_irrig=qirr)
    qsur = rt.qsur_from_rows(ptr, col, w, rows_out[hy.QFLX_SURF], rows_out[hy.QFLX_H2OSFC_SURF], G["area"])
    kw = {}
    if dam is not None:
        kw["dam"] = dict(tab=dam["tab"], res=river["res"], krls=river["krls"], month=dam["month"], begins=dam["begins"])
        if qirr is not None:
            kw["dam"]["withdrawal"] = (regrid.apply_aggregate(ptr, col, w, wb[hy.WB_QRUNOFF], 0.0), regrid.apply_aggregate(ptr, col, w, qirr, 0.0))
    if on:
        kw["land"] = rt.land_from_rows(ptr, col, w, fpi[hy.FPI_QFLX_DRAIN])
    r = rt.kinematic_call(river["wh"], river["wt"], river["volr"], qin, qsur, G["area"], G["p"], up, dt, nsub, flood=(tab, river["wf"]), **kw)
    new = dict(wh=r[0], wt=r[1], volr=r[2], qout=r[3], wf=r[4], depth=r[5], frac=r[6], qin=qin, qsur=qsur)
    k = 7
    if dam is not None:
        new.update(res=r[7], krls=r[8], take=r[9], qin=r[10])
        k = 11
    return g, rows_out, frost_out, fpi, wb, new, (r[k] if on else None)


def host_fields(cols):
    """The fields host_step reads, from the generator's columns: float64 copies, and the step's water mass at its start."""
    names = set(STEP_FIELDS + hy.WB_READS + ("t_soisno",))
    return {k: np.array(cols[k], dtype=np.float64 if np.asarray(cols[k]).dtype.kind == "f" else None) for k in names}


def begin(f, rows, wb=None):
    """The start of a host step: dtbegin_column_h2o is the columns' water mass of this moment, and W0."""
    f = dict(f)
    f["dtbegin_column_h2o"] = water_mass(f)
    return f, hy.water_balance_begin(f, rows, wb)


def river0(G, spin=True, dt=DT, nsub=NSUB):
    """The river's rows at the chain's start: G's storages and, spin, one routing call without land input behind them, which fills
    FLOOD_FRAC (elmk_routing_inundation_init leaves it zero)."""
    n = G["ncells"]
    r = dict(wh=G["wh"], wt=G["wt"], volr=G["volr"], wf=G["wf"], frac=np.zeros(n))
    if spin:
        tab = rt.inundation_tables(G["area"], G["p"], G["rdepth"], G["eprof"])
        z = np.zeros(n)
        o = rt.kinematic_call(r["wh"], r["wt"], r["volr"], z, z, G["area"], G["p"], rt.upstream_map(G["down"]), dt, nsub, flood=(tab, r["wf"]))
        r = dict(wh=o[0], wt=o[1], volr=o[2], wf=o[4], frac=o[6])
    return r


# ---- closed systems for the budget tests ------------------------------------------------------------------------------------------------
def storm_case(ncol_per_cell=3, seed=11):
    """The eight-cell storm chain of inundation_cases with ncol_per_cell columns under every cell, weights 1 / ncol_per_cell: thawed,
    snow-free loam columns whose only external terms are rain (forc_rain = qflx_top_soil) and ground evaporation (qflx_evap_tot =
    qflx_evap_grnd), so that what W4 calls the input is what the hydrology is given.  Returns the case dict (as `case`) and the fields."""
    from tests.hydrology_cases import column as loam

    down, area, p, rdepth, eprof = ic.storm_chain()
    ncells = down.size
    ncols = ncells * ncol_per_cell
    rng = np.random.default_rng(seed)
    ptr = (np.arange(ncells + 1) * ncol_per_cell).astype(np.int64)
    col = rng.permutation(ncols).astype(np.int32)
    w = np.full(ncols, 1.0 / ncol_per_cell)
    c = loam()
    N = hy.N
    f = {}
    lev = lambda a, tail=0.0: np.concatenate([np.zeros(hy.NLEVSNO), np.asarray(a, dtype=np.float64), np.full(20 - hy.NLEVSNO - len(a), tail)])  # noqa: E731
    f["h2osoi_liq"] = np.tile(lev(c["liq"]), (ncols, 1)) * rng.uniform(0.6, 1.2, (ncols, 1))
    f["h2osoi_ice"] = np.zeros((ncols, 20))
    f["dz"] = np.tile(lev(c["dz"], 1.0), (ncols, 1))
    f["zsoi"] = np.tile(lev(c["z"], 10.0), (ncols, 1))
    f["zisoi"] = np.tile(np.concatenate([np.zeros(hy.NLEVSNO), np.asarray(c["zi"]), np.full(21 - hy.NLEVSNO - N - 1, 10.0)]), (ncols, 1))
    for k in ("watsat", "sucsat", "bsw"):
        f[k] = np.tile(np.concatenate([np.asarray(c[k]), np.full(15 - N, c[k][0])]), (ncols, 1))
    f["h2osoi_vol"] = np.zeros((ncols, 15))
    f["qflx_rootsoi"] = np.zeros((ncols, 15))
    f["snl"] = np.zeros(ncols, np.int32)
    for k in ("h2osfc", "frac_h2osfc", "frac_sno_eff", "qflx_ev_soil", "qflx_ev_h2osfc", "qflx_dew_grnd", "qflx_dew_snow", "qflx_sub_snow",
              "h2ocan", "h2osno", "qflx_snwcp_liq", "qflx_snwcp_ice", "forc_snow"):
        f[k] = np.zeros(ncols)
    f["qflx_evap_grnd"] = rng.uniform(0.0, 2.0e-5, ncols)
    f["qflx_evap_tot"] = f["qflx_evap_grnd"].copy()
    f["qflx_top_soil"] = np.zeros(ncols)
    f["forc_rain"] = np.zeros(ncols)
    rows = np.zeros((hy.NROWS, ncols))
    rows[hy.ZWT], rows[hy.WA] = rng.uniform(2.0, 6.0, ncols), 4000.0
    rows[hy.HKSAT:hy.HKSAT + N] = rng.uniform(2.0e-3, 2.0e-2, (N, ncols))
    rows[hy.WTFACT], rows[hy.H2OSFC_THRESH], rows[hy.K_WET], rows[hy.RSUB_TOP_MAX] = 0.3, 5.0, 0.05, 1.0e-4
    G = dict(shape="storm", ncols=ncols, ncells=ncells, map=(ptr, col, w), cellof=cellof(ncols, ptr, col), down=down, ddist=np.full(ncells, 1.0e4),
             area=area, p=p, rdepth=rdepth, eprof=eprof, volr=np.zeros(ncells), wh=np.zeros(ncells), wt=np.zeros(ncells), wf=np.zeros(ncells),
             rows=rows, frost=None, nanq=-1)
    return G, f


def set_rain(f, rate):
    """Rain of `rate` mm/s on every column, all of it reaching the soil."""
    f = dict(f)
    f["qflx_top_soil"] = np.full(f["snl"].shape[0], float(rate))
    f["forc_rain"] = f["qflx_top_soil"].copy()
    return f
