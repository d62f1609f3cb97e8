"""The inputs of the command areas' tests, host and device (include/elmk.h "command areas"): on top of the reservoirs' cases
(tests/reservoir_cases.py) the cells' dependency rows - which dams a cell hangs on, with which shares and claims - laid out so that
every item of the census occurs in every call, the census itself, one dam with thousands of dependents, the edge values in dams and
cells of their own, and a dam above a dry crop cell on a chain.

k_command_allot takes CMD_DAMS = 64 consecutive dams per workgroup and walks their terms in tiles of CMD_TILE = 1024: the 1001-cell
case has 143 dams, three workgroups, and the 2300-cell case one dam of 2100 terms, a span of more than two tiles."""
import numpy as np

from elmkernels_amd import routing as rt
from tests import reservoir_cases as rc

NDEP = rt.NDEP
CMD_DAMS, CMD_TILE = 64, 1024
CENSUS = ("limited", "unlimited", "W = 0", "no terms", "at or below SMIN", "one slot", "two slots", "four slots", "limited and unlimited",
          "dam cell depends", "rest <= 0")
RICH, POOR, DRY = (2, 10), (3, 4, 5, 6, 7), (8,)  # reservoir_cases.dam_values' roles: storage far above SMIN, next to none, below it


def command_values(n, seed, active):
    """dam int32 [4, n], share and claim [4, n] over dams_of(n).  active: bool [n], the cells whose withdrawal is > 0.
    With j the place of a dam in the dam list and its role j % 12: dam 0 is kept without terms and dam 1 is named only by cells that
    withdraw nothing (W = 0 with terms).  A cell c takes by c % 8:
      0, 6  no slot;   1, 5  one slot, the next dam behind it;   4  one slot: an idle cell names dam 1, any other the next dam;
      2, 7  two slots: the next dam of a role with storage far above SMIN and the next with next to none - a limited and an unlimited
            dam at once where the cell withdraws;   3  four slots, the next four dams.
    Dam cells take slots like any other cell (never themselves).  Shares are random and sum to at most 1; a dam's claims are 0.9
    divided evenly among its terms.  Fewer than six dams: every cell but the dams names the first dam (one slot)."""
    rng = np.random.default_rng(seed)
    dams = dams_of(n)
    dam = np.full((NDEP, n), -1, np.int32)
    share, claim = np.zeros((NDEP, n)), np.zeros((NDEP, n))
    nd = dams.size
    if n < 2 or nd == 0:
        return dam, share, claim
    if nd < 6:
        for c in range(n):
            if c not in dams:
                dam[0, c], share[0, c] = dams[0], rng.uniform(0.3, 1.0)
    else:
        usable = np.arange(2, nd)
        role = np.arange(nd) % rc.NROLES

        def following(c, k, roles=None):
            """The k next usable dams behind cell c (wrapping), of `roles` if given, the cell itself left out."""
            pool = usable if roles is None else usable[np.isin(role[usable], roles)]
            start = int(np.searchsorted(dams[pool], c, side="right"))
            out = []
            for i in range(pool.size):
                d = int(dams[pool[(start + i) % pool.size]])
                if d != c:
                    out.append(d)
                if len(out) == k:
                    break
            return out

        for c in range(n):
            kind = c % 8
            if kind in (0, 6):
                continue
            if kind == 4 and not active[c] and c != dams[1]:
                picks = [int(dams[1])]
            elif kind in (1, 4, 5):
                picks = following(c, 1)
            elif kind in (2, 7):
                picks = following(c, 1, RICH) + following(c, 1, POOR)
            else:
                picks = following(c, 4)
            s = rng.uniform(0.2, 1.0, len(picks))
            s = s / s.sum() * rng.uniform(0.5, 0.999)
            for k, d in enumerate(picks):
                dam[k, c], share[k, c] = d, s[k]
        if n >= 16:
            share[:, 11] = np.where(dam[:, 11] >= 0, 0.25, 0.0)  # cell 11 (four slots): shares that sum to exactly 1.0
    cnt = np.bincount(dam[dam >= 0], minlength=n)
    claim = np.where(dam >= 0, 0.9 / np.maximum(cnt[np.maximum(dam, 0)], 1), 0.0)
    return dam, share, claim


def census(cmd, tab, want, allot, ratio):
    """Which items of CENSUS one call held: name -> count.  cmd: routing.command_tables; want: C1's row; allot: the dict command_allot
    filled; ratio: C2's row."""
    nslot = (cmd["DAM"] >= 0).sum(axis=0)
    lim, unl = allot["limited"], allot["unlimited"]
    two = nslot >= 2
    d0, d1 = np.maximum(cmd["DAM"][0], 0), np.maximum(cmd["DAM"][1], 0)
    both = two & (want > 0.0) & ((lim[d0] & unl[d1]) | (unl[d0] & lim[d1]))
    out = {k: int(allot[k].sum()) for k in CENSUS[:5]}
    out.update({"one slot": int((nslot == 1).sum()), "two slots": int((nslot == 2).sum()), "four slots": int((nslot == 4).sum()),
                "limited and unlimited": int(both.sum()), "dam cell depends": int((tab["DAM"] & cmd["HAS"]).sum()),
                "rest <= 0": int((cmd["HAS"] & ~(want > 0.0)).sum())})
    return out


def single_dam(n=2300, at=1150, ndeps=2100, seed=7):
    """One dam, in cell `at`, and ndeps dependents around it: its span is longer than two tiles of k_command_allot.  Returns the four
    inputs of elmk_routing_reservoir_enable, the initial RES and KRLS, and the three rows."""
    assert ndeps > 2 * CMD_TILE and ndeps < n
    rng = np.random.default_rng(seed)
    cap, beta, mstart = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    target, res, krls = np.zeros((12, n)), np.zeros(n), np.ones(n)
    cap[at], beta[at], target[:, at], res[at] = 1.0e9, 1.0, 0.0, 1.0e8 + 4.0e5  # holds its water, a little above SMIN: limited
    deps = np.delete(np.arange(n), at)[:ndeps]
    dam = np.full((NDEP, n), -1, np.int32)
    share, claim = np.zeros((NDEP, n)), np.zeros((NDEP, n))
    dam[0, deps], share[0, deps], claim[0, deps] = at, rng.uniform(0.2, 1.0, ndeps), 0.9 / ndeps
    return (cap, target, beta, mstart, res, krls), (dam, share, claim)


# ---- the edge values (C8) ------------------------------------------------------------------------------------------------------------------
EDGE_DAM0 = 17  # RES's edge values stand in dams of cells 17, 19 .. 31, each with the dependent cell behind it (18, 20 .. 32)
EDGE_INF_CELL, EDGE_NAN_CELL = 3, 6  # the cells whose only columns are columns 5 and 9 (routing_kinematic_cases.cell_map)
EDGE_INF_DAM, EDGE_INF_PEER, EDGE_ZERO_DAM = 40, 42, 44


def edge_values(n=257):
    """Dams and cells of their own on a network of outlets: the dam of cell EDGE_DAM0 + 2 i holds SPECIAL[i] in RES and supplies cell
    EDGE_DAM0 + 2 i + 1; the dam of cell EDGE_INF_DAM (RES far above SMIN) supplies EDGE_INF_CELL, whose withdrawal is infinite, and
    EDGE_INF_PEER, an ordinary cell; the dam of cell EDGE_ZERO_DAM supplies only cell 0, which has no columns (W = 0 with terms), and the
    cell EDGE_NAN_CELL, whose runoff is NaN and which withdraws nothing.  Returns the reservoirs' inputs with RES and KRLS, and the three rows."""
    cap, beta, mstart = np.zeros(n), np.zeros(n), np.zeros(n, np.int32)
    target, res, krls = np.zeros((12, n)), np.zeros(n), np.ones(n)
    dam = np.full((NDEP, n), -1, np.int32)
    share, claim = np.zeros((NDEP, n)), np.zeros((NDEP, n))
    for i, v in enumerate(rc.SPECIAL):
        d = EDGE_DAM0 + 2 * i
        cap[d], beta[d], res[d] = 1.0e9, 1.0, v
        dam[0, d + 1], share[0, d + 1], claim[0, d + 1] = d, 1.0, 0.5
    for d in (EDGE_INF_DAM, EDGE_ZERO_DAM):
        cap[d], beta[d], res[d] = 1.0e9, 1.0, 5.0e8
    for c in (EDGE_INF_CELL, EDGE_INF_PEER):
        dam[0, c], share[0, c], claim[0, c] = EDGE_INF_DAM, 1.0, 0.25
    for c in (0, EDGE_NAN_CELL):
        dam[0, c], share[0, c], claim[0, c] = EDGE_ZERO_DAM, 1.0, 0.25
    return (cap, target, beta, mstart, res, krls), (dam, share, claim)


# ---- a dam above a dry crop cell -------------------------------------------------------------------------------------------------------------
def dry_chain(n=4, dam=0, crop=3):
    """A chain of n cells of 100 km2 with the demo's parameters, cell c into c + 1: a full reservoir in cell `dam`, held back (BETA 1,
    TARGET 0: it releases a tenth of its inflow), and a crop cell `crop` whose withdrawal is far more than the little runoff brings.
    Returns (down, area, params, (cap, target, beta, mstart, res, krls), (dam rows), rn, i): rn and i are R1's aggregates, mm/s."""
    down = np.append(np.arange(1, n), -1).astype(np.int32)
    area = np.full(n, 1.0e8)
    p = np.repeat(np.array(rc.BASE)[:, None], n, axis=1)
    cap, beta, mstart = np.zeros(n), np.ones(n), np.zeros(n, np.int32)
    target, res, krls = np.zeros((12, n)), np.zeros(n), np.ones(n)
    cap[dam], res[dam] = 1.0e9, 8.0e8
    rows = np.full((NDEP, n), -1, np.int32), np.zeros((NDEP, n)), np.zeros((NDEP, n))
    rows[0][0, crop], rows[1][0, crop], rows[2][0, crop] = dam, 1.0, 0.5
    rn = np.full(n, 1.0e-7)  # 0.01 m3/s per cell
    i = np.zeros(n)
    i[crop] = 2.0e-5  # 2 m3/s: 1.7e5 m3 a day
    return down, area, p, (cap, target, beta, mstart, res, krls), rows, rn, i


def ring_values(cap, second=4, claims=(0.2, 0.1)):
    """Rows for any set of dams: every cell names the next dam behind it (wrapping, never itself) with share 0.6 and claim claims[0], and
    every `second`-th cell the dam after that as well, with share 0.3 and claim claims[1]."""
    n = cap.size
    dams = np.nonzero(cap > 0.0)[0]
    dam = np.full((NDEP, n), -1, np.int32)
    share, claim = np.zeros((NDEP, n)), np.zeros((NDEP, n))
    if dams.size < 3:
        return dam, share, claim
    for c in range(n):
        j = int(np.searchsorted(dams, c, side="right"))
        picks = [int(dams[(j + k) % dams.size]) for k in range(3)]
        picks = [d for d in picks if d != c][:2 if c % second == 0 else 1]
        for k, d in enumerate(picks):
            dam[k, c], share[k, c], claim[k, c] = d, (0.6, 0.3)[k], claims[k]
    return dam, share, claim


def reservoir_values(n, seed):
    """reservoir_cases.dam_values, and at two cells - where that has no dam - a dam in cell 0 (which has no columns) that cell 1 can
    hang on."""
    cap, target, beta, mstart, res, krls = rc.dam_values(n, seed)
    if n == 2:
        cap[0], res[0], beta[0], mstart[0], target[:, 0] = 1.0e9, 5.0e8, 0.5, 0, 20.0
    return cap, target, beta, mstart, res, krls


def dams_of(n):
    """The dams command_values lays its rows over: reservoir_cases.dam_cells, and cell 0 of a grid of two."""
    return np.array([0]) if n == 2 else rc.dam_cells(n) if n > 1 else np.array([], np.int64)


def cell_map(ncells, seed):
    """inundation_cases.cell_map, but at two cells one in which cell 1 is sure to withdraw: cell 0 (the dam's) has no columns and cell 1
    holds the forty even columns below 80."""
    from tests import inundation_cases as ic
    if ncells != 2:
        return ic.cell_map(ncells, seed)
    col = np.arange(0, 80, 2).astype(np.int32)
    return np.array([0, 0, col.size], np.int64), col, np.random.default_rng(seed).uniform(0.05, 1.5, col.size)
