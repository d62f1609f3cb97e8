"""What the river stage's device tests share (tests/test_gpu_routing*.py, tests/cell_history_cases.py): the prepared context the chained
calls run on, the small readers and comparisons around it, and the case of the run tests - 193 columns on 65 cells - with one
run_context that switches on exactly the parts a test names.  The inputs themselves come from the cases modules of the parts
(routing_kinematic_cases, inundation_cases, reservoir_cases, heat_cases)."""
import numpy as np

from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import regrid
from elmkernels_amd import routing as rt
from tests import heat_cases as hc
from tests import inundation_cases as ic
from tests import reservoir_cases as rc
from tests import routing_kinematic_cases as kc
from tests.hydrology_cases import _new, clear_snow, prepare
from tests.run_cases import DT, NREC, _inputs, snapshot, upload_series

TOL = 1.0e-9
NAN = float("nan")
NCOL, NCELL, NSTEPS = 193, 65, 6  # the run case: 65 cells are one past the 64-cell padding
PARTS = ("routing", "kinematic", "inundation", "reservoir", "heat")  # in the order the entry points require


# ---- the context of the chained calls -------------------------------------------------------------------------------------------------
def base():
    """The columns of the chained calls and the hydrology's prepared rows."""
    b = _inputs(kc.NCOLS, 611)
    clear_snow(b[0])
    return b, prepare(b[0], 612)


def context(base, lib_path, ncells, seed=3, cell_map=kc.cell_map, hydrology=True, withdraw=False):
    """The prepared context with the water balance and an output grid of ncells cells (cell_map(ncells, seed), kept as D._map).
    hydrology: the stage stepped once so that its surface rows hold values (D._surf).  withdraw: the irrigation enabled with no
    irrigated column and a rate that applies for the whole test, stepped once so that its QFLX_IRRIG row holds it (D._qirr)."""
    b, rows = base
    D = _new(b[0], b[1], b[2], rows, lib_path, b[3], b[4])
    D.water_balance_enable(TOL)
    ptr, col, w = cell_map(ncells, seed)
    D.set_output_grid(ptr, col, w, fill=NAN)
    D._map = (ptr, col, w)
    D._qirr = None
    if withdraw:
        D.irrigation_enable(np.full(kc.NCOLS, ir.NOT_IRRIGATED, np.int32))
        rate = np.where(np.arange(kc.NCOLS) % 2 == 0, np.random.default_rng(9).uniform(0.0, 3.0e-5, kc.NCOLS), 0.0)
        D.irrigation_init(rate, np.full(kc.NCOLS, 1000.0))
        D.irrigation(DT, 0)
        D._qirr = D.irrigation_read(ir.QFLX_IRRIG)
        assert (D._qirr > 0.0).any()
    if hydrology:
        D.soil_hydrology(DT)
        D._surf = (D.soil_hydrology_read(hy.QFLX_SURF), D.soil_hydrology_read(hy.QFLX_H2OSFC_SURF))
    return D


def set_runoff(D, q):
    """q through the water balance: the QRUNOFF row the next call reads."""
    D.upload("qflx_snwcp_liq", q)
    D.water_balance(DT)
    return D.water_balance_read(hy.WB_QRUNOFF)


def read_rows(D, rows):
    return [D.routing_read(w) for w in rows]


def host_inputs(D, qrunoff, area):
    """K1's QIN (the withdrawal included where it is on) and QSUR, and R1's two aggregates for D2 (None without the withdrawal)."""
    ptr, col, w = D._map
    qin = rt.qin_from_rows(ptr, col, w, qrunoff, area, qflx_irrig=D._qirr)
    wd = None
    if D._qirr is not None:
        wd = (regrid.apply_aggregate(ptr, col, w, qrunoff, 0.0), regrid.apply_aggregate(ptr, col, w, D._qirr, 0.0))
    return qin, rt.qsur_from_rows(ptr, col, w, D._surf[0], D._surf[1], area), wd


def differing(g, want):
    return np.nonzero(g.view(np.uint64) != want.view(np.uint64))[0][:5]


def finite(x, fill=7.0):
    return np.where(np.isfinite(x) & (np.abs(x) < 1e200), x, fill)


def river_snapshot(D, rows):
    """Every non-series field, the hydrology's and the water balance's rows and, with rows, those routing rows and the count."""
    more = {"route": np.stack(read_rows(D, rows)), "count": np.array(D.routing_count())} if rows else {}
    return snapshot(D, hyd=D.soil_hydrology_rows(), wb=D.water_balance_rows(), **more)


# ---- the run case ----------------------------------------------------------------------------------------------------------------------
def run_case(flood=False, dam=False, heat=False):
    """The columns, their records and prepared rows, the map of 193 columns onto 65 cells, the forest, and the cell values: a dict.
    volr, wh, wt: the kinematic scheme's edge storages made finite.  flood (and dam, whose case has the floodplain too): the
    inundation's inputs, which move p and the three storages (inundation_cases.flood_values).  dam: the reservoirs', with February's
    targets other than January's and every other dam's year beginning in February.  heat: the shade and the two temperatures."""
    b = _inputs(NCOL, 531)
    clear_snow(b[0])
    rows = prepare(b[0], 532)
    rng = np.random.default_rng(77)
    cnt = rng.integers(0, 6, NCELL)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = rng.integers(0, NCOL, int(ptr[-1])).astype(np.int32)
    m = (ptr, col, rng.uniform(0.1, 1.0, col.size))
    ddist, area, p, volr, wh, wt = kc.cell_values(NCELL, 78)
    volr, wh, wt = finite(volr), finite(wh), finite(wt)
    G = dict(b=b, rec=b[5], rows=rows, map=m, down=kc.networks(NCELL, 79)["forest"], ddist=ddist, area=area)
    if flood or dam:
        G["rdepth"], G["eprof"], p, volr, wh, wt, wf = ic.flood_values(NCELL, 80, area, p, volr, wh, wt, 3, DT)
        G["wf"] = finite(wf)
    if dam:
        cap, target, beta, mstart, res, krls = rc.dam_values(NCELL, 81)
        dams = rc.dam_cells(NCELL)
        target[1, dams] = 2.0 * target[0, dams] + 25.0
        mstart[dams[::2]] = 1
        G["dam"] = (cap, target, beta, mstart, finite(res), krls)
    if heat:
        G["shade"], tt, tr = hc.heat_values(NCELL, 81)
        G["temps"] = tuple(np.where((x > 200.0) & (x < 400.0), x, 280.0) for x in (tt, tr))
    G.update(p=p, volr=volr, wh=wh, wt=wt)
    return G


def run_context(G, graph, lib_path=None, parts=PARTS[:1], nsub=3, init=True):
    """A run context over run_case's G, reserved for two runs of NSTEPS steps with the series uploaded, the water balance and the
    output grid on, and exactly `parts` enabled and (init) initialised from G."""
    b = G["b"]
    D = _new(b[0], b[1], b[2], G["rows"], lib_path, b[3], b[4])
    D.set_graph(graph)
    D.run_reserve(NREC, 2 * NSTEPS)
    upload_series(D, G["rec"])
    D.water_balance_enable(TOL)
    D.set_output_grid(*G["map"], fill=NAN)
    assert set(parts) <= set(PARTS)
    enable = {"routing": lambda: D.routing_enable(G["down"], G["ddist"], G["area"], rt.EFFVEL, nsub),
              "kinematic": lambda: D.routing_kinematic_enable(G["p"]),
              "inundation": lambda: D.routing_inundation_enable(G["rdepth"], G["eprof"]),
              "reservoir": lambda: D.routing_reservoir_enable(*G["dam"][:4]),
              "heat": lambda: D.routing_heat_enable(hc.SUBLEV, G["shade"])}
    start = {"routing": lambda: D.routing_init(G["volr"]),
             "kinematic": lambda: D.routing_kinematic_init(G["wh"], G["wt"]),
             "inundation": lambda: D.routing_inundation_init(G["wf"]),
             "reservoir": lambda: D.routing_reservoir_init(*G["dam"][4:]),
             "heat": lambda: D.routing_heat_init(*G["temps"])}
    for calls in (enable, start) if init else (enable,):
        for part in PARTS:
            if part in parts:
                calls[part]()
    return D
