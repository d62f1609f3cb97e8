"""The inputs of the cell-row history tests (include/elmk.h "cell rows on history tapes"): one small context with the soil hydrology, the
water balance, an output grid in which every column lies in at most one cell, the irrigation with its river supply limit, the routing
with the withdrawal, the kinematic-wave scheme and its floodplain inundation - the river stages whose cell rows the entries sample -,
the step the tests chain (irrigation with the limit behind it, a prepared runoff row through the water balance, the routing, the history
sample), and the entries: every op over VOLR, QOUT, WF, FLOOD_FRAC and UNMET_SUM on two tapes, beside one entry of each older kind."""
import numpy as np

from elmkernels_amd import history as hs
from elmkernels_amd import hydrology as hy
from elmkernels_amd import irrigation as ir
from elmkernels_amd import routing as rt
from tests import inundation_cases as ic
from tests import irrigation_supply_cases as sc
from tests.river_cases import finite  # noqa: F401 (the tests take it from here)

DT = 1800.0
TOL, THR = 1.0e-9, 0.1
NAN = float("nan")
OPS = ("avg", "sum", "max", "min", "inst")
# (family, which, the name in messages); the tape of entry (row i, op j) is (i + j) % 2
CELL_ROWS = (("routing", rt.VOLR, "VOLR"), ("routing", rt.QOUT, "QOUT"), ("routing", rt.WF, "WF"), ("routing", rt.FLOOD_FRAC, "FLOOD_FRAC"),
             ("supply", ir.UNMET_SUM, "UNMET_SUM"))
LINEAR_ROWS = CELL_ROWS[:2]  # what the linear scheme alone has of them


def river_case(ncols, ncells, seed, cells_with_columns=None):
    """The columns (the irrigation's generated tier with the hydrology's prepared rows) and everything that lives on cells: a dict.
    cells_with_columns: only that many cells, spread over the grid, hold columns - the others are pass-through reaches; else every cell
    but cell 0 (of a grid of more than eight cells) holds two or more.  VOLR, WH, WT and WF carry the kinematic-wave and inundation
    tests' edge values - NaN, +-inf, a negative storage, 1e300, -0.0 and a subnormal - each in a cell of its own where there are cells
    enough."""
    from tests.hydrology_cases import clear_snow, prepare
    from tests.irrigation_cases import generated

    cols, scal, soil, sched = generated(ncols, seed)
    clear_snow(cols)
    rows = prepare(cols, seed + 1)
    if cells_with_columns is None:
        empty = (0,) if ncells > 8 else ()
    else:
        keep = set(np.linspace(1, ncells - 1, cells_with_columns).astype(int).tolist())
        empty = tuple(c for c in range(ncells) if c not in keep)
    m = sc.cell_map(ncols, ncells, seed + 2, empty=empty, free=3)
    ddist, area, p0, volr0, wh0, wt0 = ic.cell_values(ncells, seed + 3)
    rdepth, eprof, p, volr, wh, wt, wf = ic.flood_values(ncells, seed + 4, area, p0, volr0, wh0, wt0, 2, DT)
    nets = ic.networks(ncells, seed + 5)
    c = np.arange(ncols)
    rate0 = np.where(sched >= 0, 1.0e-4 + 1.0e-6 * (c % 97), 0.0)
    nleft0 = np.where(c % 3 == 0, (c % 7).astype(np.float64), 0.0)
    rng = np.random.default_rng(seed + 6)
    runoff = [rng.uniform(0.0, 4.0e-5, ncols) for _ in range(3)]
    return dict(ncols=ncols, ncells=ncells, cols=cols, scal=scal, soil=soil, sched=sched, rows=rows, map=m, ddist=ddist, area=area,
                params=p, rdepth=rdepth, eprof=eprof, volr=volr, wh=wh, wt=wt, wf=wf, down=nets.get("forest", nets["outlets"]),
                rate0=rate0, nleft0=nleft0, runoff=runoff)


def context(G, lib_path=None, kinematic=True, flood=True, supply=True, routing=True, init=True, nsub=2):
    """A context over river_case's G with the river stages on (each switch takes one off, and what needs it with it)."""
    from tests.hydrology_cases import _new

    D = _new(G["cols"], G["scal"], G["soil"], G["rows"], lib_path)
    D.water_balance_enable(TOL)
    D.set_output_grid(*G["map"], fill=NAN)
    D.irrigation_enable(G["sched"])
    if init:
        D.irrigation_init(G["rate0"], G["nleft0"])
    if routing:
        enable_routing(D, G, kinematic, flood, supply, init, nsub)
    return D


def enable_routing(D, G, kinematic=True, flood=True, supply=True, init=True, nsub=2):
    D.routing_enable(G["down"], G["ddist"], G["area"], rt.EFFVEL, nsub)
    D.routing_set_withdrawal(True)
    if kinematic:
        D.routing_kinematic_enable(G["params"])
    if kinematic and flood:
        D.routing_inundation_enable(G["rdepth"], G["eprof"])
    if supply:
        D.irrigation_supply_enable(THR)
    if init:
        D.routing_init(G["volr"])
        if kinematic:
            D.routing_kinematic_init(G["wh"], G["wt"])
        if kinematic and flood:
            D.routing_inundation_init(G["wf"])


def step(D, G, k, dt=DT, sample=True):
    """Step k of a chain: the irrigation at half past five plus k steps (the limit's launch follows it), runoff row k % 3 through the
    water balance, the routing, the history sample."""
    D.irrigation(dt, int(5 * 3600 + 1800 * (k + 1)) % 86400)
    D.upload("qflx_snwcp_liq", G["runoff"][k % 3])
    D.water_balance(dt)
    D.routing(dt)
    if sample:
        D.history_accumulate()


def add_cell_entries(D, rows=CELL_ROWS, ops=OPS):
    """Every op over every row of `rows`, spread over tapes 0 and 1: {(name, op): (entry, tape)}."""
    ids = {}
    for i, (fam, which, name) in enumerate(rows):
        for j, op in enumerate(ops):
            tape = (i + j) % 2
            ids[(name, op)] = (D.cell_history_add_row(tape, fam, which, op), tape)
    return ids


def add_other_entries(D):
    """One entry of each older kind, so that one launch carries every kind of row: a state field of ten levels on tape 0, a column row
    on tape 1, a gridded field on tape 0 and a gridded row on tape 1.  [(entry, tape)]."""
    return [(D.history_add(0, "h2osoi_liq", "avg"), 0), (D.history_add_row(1, "water_balance", hy.WB_QRUNOFF, "max"), 1),
            (D.gridded_history_add(0, "t_grnd", "min"), 0), (D.gridded_history_add_row(1, "irrigation", ir.QFLX_IRRIG, "sum"), 1)]


def read_cell_rows(D, rows=CELL_ROWS):
    """The sampled rows as the read calls return them: {name: float64 [ncells]}."""
    return {name: (D.routing_read(which) if fam == "routing" else D.irrigation_supply_read(which)) for fam, which, name in rows}


def host_results(samples, rows=CELL_ROWS, ops=OPS):
    """history.fold_cell_rows over the per-step reads `samples` ([{name: row}]): {(name, op): float64 [ncells]}."""
    return {(name, op): hs.fold_cell_rows(op, [s[name] for s in samples]) for _, _, name in rows for op in ops}


def canon(a):
    """The 64-bit words of a, every NaN as the one quiet NaN: which NaN an operation on a NaN returns is the one thing IEEE 754 leaves
    to the implementation, so the host's fold and the device's agree on WHERE the NaNs are and on every other bit."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.float64("nan"), a).view(np.uint64)


def differing(got, want):
    return np.nonzero(canon(got) != canon(want))[0][:5]
