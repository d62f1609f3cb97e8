"""The inputs of the stream temperature's tests, host and device (include/elmk.h "stream temperature"): the kinematic-wave test's
builders (tests/routing_kinematic_cases.py) at the same sizes and seeds, and on top of them the heat: a cell map with a hot and a cold
cell of one column each, the column fields H1 aggregates, the shade, the initial temperatures with each edge value in a cell of its
own, the census, and the chains and pools of the physical checks."""
import numpy as np

from elmkernels_amd import routing as rt
from tests.routing_kinematic_cases import BASE, INF, NAN, NCOLS, SPECIAL, cell_map, cell_values, networks, snwcp  # noqa: F401

NCALLS = 5
CASES = ((1, 1800.0), (2, 1.0), (5, 3600.0))  # (nsub, dt): FIRST and LAST the same launch, adjacent, and apart
CENSUS_CASE = (5, 3600.0)
SUBLEV = 3
HOT_CELL, COLD_CELL, HOT_COL, COLD_COL = 7, 8, 13, 17  # cells of one column each, under a forcing that drives them past TMAX and below TFRZ
PA0_CELL, TANAN_CELL, PA0_COL, TANAN_COL = 9, 10, 21, 23  # cells of one column each: PA == 0, and a NaN TA
PINNED = ((HOT_CELL, HOT_COL, 0.8), (COLD_CELL, COLD_COL, 1.1), (PA0_CELL, PA0_COL, 1.0), (TANAN_CELL, TANAN_COL, 0.7))
TT_EDGE0, TR_EDGE0 = 57, 74  # TT's edge values stand in cells 57, 59 .. 71, TR's in 74, 76 .. 88
FIELDS = ("forc_tbot", "forc_pbot", "forc_qbot", "forc_lwrad", "forc_u", "forc_v", "forc_solad", "forc_solai", "t_grnd", "t_soisno")


def heat_map(ncells, seed):
    """routing_kinematic_cases.cell_map with the cells of PINNED holding one column each, which no other cell holds, where there are
    cells enough."""
    ptr, col, w = cell_map(ncells, seed)
    if ncells <= TANAN_CELL:
        return ptr, col, w
    col = np.where(np.isin(col, [k for _, k, _ in PINNED]), 19, col)
    cells = [(col[ptr[c]:ptr[c + 1]], w[ptr[c]:ptr[c + 1]]) for c in range(ncells)]
    for c, k, x in PINNED:
        cells[c] = (np.array([k]), np.array([x]))
    ptr = np.concatenate([[0], np.cumsum([k.size for k, _ in cells])]).astype(np.int64)
    return ptr, np.concatenate([k for k, _ in cells]).astype(np.int32), np.concatenate([x for _, x in cells])


def columns(ncols, seed, call=0, edges=True):
    """The column fields of H1, float64 in the host layout ([ncols] and [ncols, nlev]): a spread of summer and winter air over ground on
    both sides of TFRZ; column HOT_COL under a longwave that no water stands, column COLD_COL under a gale of 200 K; column 21 with
    PA == 0 and column 23 with a NaN TA (edges=False: without these two)."""
    rng = np.random.default_rng(seed + 17 * call)
    ta = rng.uniform(255.0, 305.0, ncols)
    c = {"forc_tbot": ta, "forc_pbot": rng.uniform(6.0e4, 1.02e5, ncols), "forc_qbot": rng.uniform(1.0e-4, 1.5e-2, ncols),
         "forc_lwrad": rng.uniform(150.0, 450.0, ncols), "forc_u": rng.uniform(-8.0, 8.0, ncols), "forc_v": rng.uniform(-8.0, 8.0, ncols),
         "forc_solad": rng.uniform(0.0, 350.0, (ncols, 2)), "forc_solai": rng.uniform(0.0, 120.0, (ncols, 2)),
         "t_grnd": ta + rng.uniform(-6.0, 6.0, ncols), "t_soisno": rng.uniform(262.0, 296.0, (ncols, 20))}
    if ncols > 23:
        c["forc_lwrad"][HOT_COL] = 1.0e7
        c["forc_tbot"][COLD_COL], c["forc_u"][COLD_COL], c["forc_lwrad"][COLD_COL] = 200.0, 5000.0, 0.0
        c["forc_solad"][COLD_COL], c["forc_solai"][COLD_COL] = 0.0, 0.0
        if edges:
            c["forc_pbot"][PA0_COL] = 0.0
            c["forc_tbot"][TANAN_COL] = NAN
    return c


def as_stored(cols, f32):
    """The fields as a build stores them, widened: rounded to fp32 in the fp32-state build."""
    return {k: (np.asarray(v, np.float64).astype(np.float32).astype(np.float64) if f32 else np.asarray(v, np.float64)) for k, v in cols.items()}


def heat_values(n, seed):
    """shade [n] and the initial TT and TR: water between 274 and 300 K, with each edge value in a cell of its own where there are cells
    enough (TT's in cells 57, 59 .. 71, TR's in 74, 76 .. 88), a store below TFRZ in cell 90 and one above TMAX in cell 92."""
    rng = np.random.default_rng(seed)
    shade = np.where(rng.random(n) < 0.3, 0.0, rng.uniform(0.0, 1.0, n))
    tt, tr = rng.uniform(274.0, 300.0, n), rng.uniform(274.0, 300.0, n)
    for i, v in enumerate(SPECIAL):
        for row, first in ((tt, TT_EDGE0), (tr, TR_EDGE0)):
            if first + 2 * i < n:
                row[first + 2 * i] = v
    if n > 92:
        tt[90] = tr[90] = 250.0
        tt[92] = tr[92] = 330.0
    return shade, tt, tr


def aggregates(n, seed, call):
    """K1's QIN and QSUR (m3/s) for host tests that have no columns: QSUB of both signs."""
    rng = np.random.default_rng(seed + 31 * call)
    qin = rng.uniform(0.0, 8.0, n)
    return qin, np.where(np.arange(n) % 3 == 0, qin + rng.uniform(0.0, 2.0, n), qin * rng.uniform(0.0, 1.0, n))


def missing_branches(census):
    return [k for k in rt.HEAT_BRANCHES if not np.any(census.get(k, False))]


def passive_prep(n, tsur=None, tsub=None):
    """heat_prep's rows of cells without terms (no exchange through the surface), with the runoff's temperatures given."""
    z = np.zeros(n)
    x = {k: z.copy() for k in rt.HEAT_PREP_ROWS}
    x["TSUR"] = np.full(n, rt.TFRZ) if tsur is None else np.asarray(tsur, np.float64)
    x["TSUB"] = np.full(n, rt.TFRZ) if tsub is None else np.asarray(tsub, np.float64)
    x["TEQ"] = rt._fl(x["TA"])
    x["terms"] = np.zeros(n, bool)
    return x


def uniform_params(n):
    return np.repeat(np.array(BASE)[:, None], n, axis=1)
