"""The inputs of the river supply limit's tests, host and device (include/elmk.h "irrigation: river supply limit"): a cell map in which
every column lies in at most one cell, with the shapes the kernel can go wrong at, cell values with each edge storage in a cell of its
own, column rows that put every case of S0 - S6 into one call, and the census that shows which cases a call held."""
import numpy as np

NAN, INF = float("nan"), float("inf")
# the edge storages, each in a cell of its own (cells 8 .. 8 + len - 1 where there are cells enough)
SPECIAL_VOLR = (0.0, -0.0, -3.5e4, NAN, INF, 5e-324)
CASES = ("empty_cell", "one_term_cell", "column_in_no_cell", "vd_zero", "vd_below_avail", "vd_above_avail", "volr_zero", "volr_negative",
         "volr_nan", "volr_inf", "vc_above_volr", "mixed_cell", "checking_rate_zero")


def cell_map(ncols, ncells, seed, big=0, empty=(), single=(), free=None):
    """A CSR map of ncells cells over ncols columns, every column in at most one cell and about one in a hundred (`free`: how many) in
    none; cell `big[0]` holds big[1] columns, the cells of `empty` none, those of `single` one, and the rest is dealt out at random (at
    least two each).  The columns of a cell are in no particular order, so the rows are gathered.  Returns (ptr int64, col int32, w)."""
    rng = np.random.default_rng(seed)
    free = max(1, ncols // 100) if free is None else free
    cnt = np.full(ncells, -1, np.int64)
    cnt[list(empty)] = 0
    cnt[list(single)] = 1
    if big:
        cnt[big[0]] = big[1]
    rest = np.nonzero(cnt < 0)[0]
    left = ncols - free - int(cnt[cnt > 0].sum())
    assert left >= 2 * rest.size, "too few columns for the cells"
    cnt[rest] = 2 + rng.multinomial(left - 2 * rest.size, np.full(rest.size, 1.0 / rest.size))
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    col = rng.permutation(ncols)[:int(ptr[-1])].astype(np.int32)
    w = rng.uniform(0.05, 1.5, col.size) / np.repeat(np.maximum(cnt, 1), cnt)
    return ptr, col, w


def cell_of_column(ptr, col, ncols):
    out = np.full(ncols, -1, np.int64)
    out[col] = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    return out


def cell_values(ncells, seed, lo=3.0, hi=8.0):
    """area and VOLR: storages log-uniform in 10^lo .. 10^hi m3, so that some cells hold far more and some far less than a day's
    demand, and the edge values of SPECIAL_VOLR in cells 8 .. where there are cells enough (else from cell 1 on)."""
    rng = np.random.default_rng(seed)
    area = rng.uniform(0.5e8, 2.5e8, ncells)
    volr = 10.0 ** rng.uniform(lo, hi, ncells)
    first = 8 if ncells >= 8 + len(SPECIAL_VOLR) else 1
    for i, v in enumerate(SPECIAL_VOLR):
        if first + i < ncells:
            volr[first + i] = v
    return area, volr


def column_rows(ptr, col, ncols, nspd, seed):
    """RATE, NLEFT and QFLX_IRRIG as a step of the irrigation may leave them: one column in four checking (NLEFT = nspd, QFLX_IRRIG 0),
    one in four inside an open window (0 < NLEFT < nspd; QFLX_IRRIG = RATE, it applied in this step), one in eight whose window has
    just closed (NLEFT 0, QFLX_IRRIG = RATE), the rest idle.  Some checking columns have RATE 0; the first cell of three or more
    terms is mixed (its first term checks, its second is committed); the last cell of two or more terms only checks."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, ncols, p=[0.25, 0.25, 0.125, 0.375])
    cnt = np.diff(ptr)
    many = np.nonzero(cnt >= 3)[0]
    if many.size:
        p0 = int(ptr[many[0]])
        kind[col[p0]], kind[col[p0 + 1]] = 0, 1
    two = np.nonzero(cnt >= 2)[0]
    if two.size:
        kind[col[ptr[two[-1]]:ptr[two[-1] + 1]]] = 0
    rate = rng.uniform(5.0e-5, 2.0e-3, ncols)
    rate[(kind == 0) & (np.arange(ncols) % 5 == 0)] = 0.0
    nleft = np.zeros(ncols)
    nleft[kind == 0] = float(nspd)
    nleft[kind == 1] = rng.integers(1, max(nspd, 2), ncols)[kind == 1] if nspd > 1 else 0.0
    qirr = np.where((kind == 1) | (kind == 2), rate, 0.0)
    rate[kind == 3] = np.where(np.arange(ncols) % 2 == 0, rate, 0.0)[kind == 3]  # (an idle column keeps its last rate, or never had one)
    return rate, nleft, qirr


def census(ptr, col, ncols, volr, nleft, rate, nspd, rows):
    """Which CASES one call held: name -> count.  rows: the four rows supply_limit returned (DEMAND, COMMITTED, RATIO, UNMET_SUM)."""
    cnt = np.diff(ptr)
    cell = cell_of_column(ptr, col, ncols)
    checks = nleft == float(nspd)
    comm = ~checks & (nleft > 0.0)
    has = lambda m: np.bincount(cell[m & (cell >= 0)], minlength=cnt.size) > 0  # noqa: E731
    vd, vc, ratio = rows[0], rows[1], rows[2]
    with np.errstate(all="ignore"):
        return {"empty_cell": int((cnt == 0).sum()), "one_term_cell": int((cnt == 1).sum()), "column_in_no_cell": int((cell < 0).sum()),
                "vd_zero": int(((vd == 0.0) & (cnt > 0)).sum()), "vd_below_avail": int(((vd > 0.0) & (ratio == 1.0)).sum()),
                "vd_above_avail": int((ratio < 1.0).sum()), "volr_zero": int(((volr == 0.0) & (vd > 0.0)).sum()),
                "volr_negative": int(((volr < 0.0) & (vd > 0.0)).sum()), "volr_nan": int(((volr != volr) & (vd > 0.0)).sum()),
                "volr_inf": int(((volr == INF) & (vd > 0.0)).sum()), "vc_above_volr": int(((vc > volr) & (vd > 0.0) & (volr > 0.0)).sum()),
                "mixed_cell": int((has(checks) & has(comm)).sum()), "checking_rate_zero": int((checks & (rate == 0.0) & (cell >= 0)).sum())}
