"""The inputs of the river supply limit's tests, host and device (include/elmk.h "irrigation: river supply limit"): a cell map in which
every column lies in at most one cell, with the shapes the kernel can go wrong at, cell values with each edge storage in a cell of its
own, column rows that put every case of S0 - S6 into one call, and the census that shows which cases a call held; then the edge inputs:
rates that are NaN, infinite, huge and subnormal on checking and committed columns, the maps at the tile and workgroup boundaries of
k_irrigation_supply, and their census."""
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


# ---- the edge inputs of the limit -----------------------------------------------------------------------------------------------------
SUP_CELLS, SUP_TILE = 64, 1024  # k_irrigation_supply: cells per workgroup, terms per LDS tile
EDGE_RATES = (NAN, INF, 1e300, 1.7976931348623157e308, 5e-324, 1e-320)
EDGE_STORAGES = (None, INF, 0.0)  # None: the ordinary storage cell_values drew
SUPPLY_EDGE_CASES = ("vd_nan", "vd_inf", "vc_nan", "vc_inf", "ratio_zero_finite_vd", "ratio_zero_inf_vd", "ratio_between", "rate_becomes_nan",
                     "rate_becomes_zero", "unmet_nan", "unmet_stays", "quiet_workgroup", "limited_workgroup")


def edge_cells(ptr):
    """The cells edge_rows writes to: len(EDGE_RATES) x 2 x len(EDGE_STORAGES) cells of two or more terms from cell 14 on (behind the
    edge storages of cell_values), the last cell of two or more terms left out (column_rows makes it one that only checks)."""
    cnt = np.diff(ptr)
    cand = [int(c) for c in np.nonzero(cnt >= 2)[0] if c >= 8 + len(SPECIAL_VOLR)][:-1]
    need = len(EDGE_RATES) * 2 * len(EDGE_STORAGES)
    assert len(cand) >= need, f"{len(cand)} cells of two or more terms behind cell 13, {need} needed"
    return cand[:need]


def edge_rows(ptr, col, ncols, nspd, seed, volr):
    """column_rows, and on top of it every value of EDGE_RATES as the RATE of the first term of a cell of its own, once on a checking
    column (NLEFT = nspd, QFLX_IRRIG 0) and once on a committed one (NLEFT = nspd - 1, QFLX_IRRIG the same value: it applied in this
    step; with nspd = 1 the window has just closed and only S2's y carries the value), each in a cell of ordinary storage, in a
    cell with VOLR = +inf and in one with VOLR = 0.  The second term of the last of these cells is a column with NLEFT = nspd + 1,
    which S0 does not mark (the driver of S0's remark: a window opened at a shorter step).  Returns (rate, nleft, qirr, volr); volr is
    a copy."""
    rate, nleft, qirr = column_rows(ptr, col, ncols, nspd, seed)
    volr = np.array(volr, dtype=np.float64)
    cells = iter(edge_cells(ptr))
    longer = int(col[ptr[edge_cells(ptr)[-1]] + 1])
    rate[longer], nleft[longer] = 3.0e-4, float(nspd + 1)
    qirr[longer] = rate[longer]
    for v in EDGE_RATES:
        for committed in (False, True):
            for s in EDGE_STORAGES:
                c = next(cells)
                i = int(col[ptr[c]])
                rate[i], nleft[i], qirr[i] = v, float(nspd - 1 if committed else nspd), (v if committed else 0.0)
                if s is None:
                    assert np.isfinite(volr[c]) and volr[c] > 0.0
                else:
                    volr[c] = s
    return rate, nleft, qirr, volr


def supply_edge_census(ptr, col, ncols, nleft, rate, rate_out, nspd, rows):
    """Which SUPPLY_EDGE_CASES one call held: name -> count.  rate, nleft: what the limit read; rate_out, rows: what supply_limit
    returned.  rate_becomes_nan: a checking column's infinite rate times ratio 0; rate_becomes_zero: a positive finite rate times
    ratio 0.  unmet_stays: a cell of NaN demand is not limited - its ratio is exactly 1.0, the term it adds is Vd - Vd and the RATE
    of its checking columns keeps its bits.  quiet_workgroup: 64 consecutive cells from a multiple of 64 on, none with ratio != 1.0
    (the kernel skips S5's walk); limited_workgroup: such a group, or the ragged last one, with at least one."""
    cnt = np.diff(ptr)
    ncells = cnt.size
    cell = cell_of_column(ptr, col, ncols)
    checks = (nleft == float(nspd)) & (cell >= 0)
    vd, vc, ratio, unmet = rows
    changed = rate_out.view(np.uint64) != np.asarray(rate, dtype=np.float64).view(np.uint64)
    moved = np.bincount(cell[changed & (cell >= 0)], minlength=ncells) > 0
    groups = [ratio[g:g + SUP_CELLS] for g in range(0, ncells, SUP_CELLS)]
    with np.errstate(all="ignore"):
        return {"vd_nan": int(np.isnan(vd).sum()), "vd_inf": int((vd == INF).sum()), "vc_nan": int(np.isnan(vc).sum()),
                "vc_inf": int((vc == INF).sum()), "ratio_zero_finite_vd": int(((ratio == 0.0) & np.isfinite(vd)).sum()),
                "ratio_zero_inf_vd": int(((ratio == 0.0) & (vd == INF)).sum()), "ratio_between": int(((ratio > 0.0) & (ratio < 1.0)).sum()),
                "rate_becomes_nan": int((checks & np.isinf(rate) & np.isnan(rate_out)).sum()),
                "rate_becomes_zero": int((checks & np.isfinite(rate) & (rate > 0.0) & (rate_out == 0.0)).sum()),
                "unmet_nan": int(np.isnan(unmet).sum()), "unmet_stays": int((np.isnan(vd) & (ratio == 1.0) & ~moved).sum()),
                "quiet_workgroup": sum(1 for g in groups if g.size == SUP_CELLS and (g == 1.0).all()),
                "limited_workgroup": sum(1 for g in groups if (g != 1.0).any())}


LAYOUTS = ("tiles", "big_last", "all_empty")


def shape_map(ncells, seed, layout="tiles", lead=()):
    """A CSR map at the shapes k_irrigation_supply can go wrong at, every column in at most one cell, over just enough columns (three
    lie in no cell).  A workgroup takes 64 consecutive cells.
      "tiles":     the first workgroup's terms number exactly SUP_TILE, the second's (where there is one) exactly SUP_TILE + 1, the
                   cells behind cell 127 hold three terms each; cell 0 is empty and cell 5 holds one term where there are cells enough.
      "big_last":  the last cell of the first workgroup holds 2100 terms, more than two tiles; the second workgroup's cells (all 64 of
                   them at 129 cells) are empty, so that its span is empty (P0 == P1); cell 128 holds three terms.
      "all_empty": no cell has a term.
    lead: columns that become the first term of a cell of their own each - the cells of two or more terms from cell 14 on, in order.
    Returns (ptr int64, col int32, w, ncols)."""
    assert layout in LAYOUTS
    rng = np.random.default_rng(seed)
    cnt = np.zeros(ncells, np.int64)

    def deal(lo, hi, total):
        """Cells lo .. hi - 1 share `total` terms: cell 0 none and cell 5 one where the group has more than eight cells, the rest two or more."""
        m = hi - lo
        if m == 1:
            cnt[lo] = total
            return
        fixed = {lo: 0, lo + 5: 1} if m > 8 else {}
        for c, v in fixed.items():
            cnt[c] = v
        rest = np.array([c for c in range(lo, hi) if c not in fixed])
        left = total - sum(fixed.values())
        assert left >= 2 * rest.size
        cnt[rest] = 2 + rng.multinomial(left - 2 * rest.size, np.full(rest.size, 1.0 / rest.size))

    g0 = min(SUP_CELLS, ncells)
    if layout == "tiles":
        deal(0, g0, SUP_TILE)
        if ncells > SUP_CELLS:
            deal(SUP_CELLS, min(2 * SUP_CELLS, ncells), SUP_TILE + 1)
        cnt[2 * SUP_CELLS:] = 3
        assert int(cnt[:g0].sum()) == SUP_TILE and (ncells <= SUP_CELLS or int(cnt[SUP_CELLS:2 * SUP_CELLS].sum()) == SUP_TILE + 1)
    elif layout == "big_last":
        if g0 > 1:
            deal(0, g0 - 1, 4 * (g0 - 1))
        cnt[g0 - 1] = 2100
        cnt[2 * SUP_CELLS:] = 3
        assert int(cnt[g0 - 1]) > 2 * SUP_TILE and not cnt[SUP_CELLS:2 * SUP_CELLS].any()
        assert ncells < 2 * SUP_CELLS or cnt[SUP_CELLS:2 * SUP_CELLS].size == SUP_CELLS
    else:
        assert not cnt.any()
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nnz = int(ptr[-1])
    ncols = max(nnz + 3, 65)
    lead = [int(i) for i in lead]
    assert len(set(lead)) == len(lead) and all(0 <= i < ncols for i in lead)
    others = rng.permutation(np.setdiff1d(np.arange(ncols), lead))
    col = np.full(nnz, -1, np.int64)
    own = [int(c) for c in np.nonzero(cnt >= 2)[0] if c >= 8 + len(SPECIAL_VOLR)][:len(lead)]
    assert len(own) == len(lead), "too few cells for the leading columns"
    col[ptr[own]] = lead
    col[col < 0] = others[:nnz - len(lead)]
    assert np.unique(col).size == nnz and (np.diff(ptr) == cnt).all()
    w = rng.uniform(0.05, 1.5, nnz) / np.repeat(np.maximum(cnt, 1), cnt)
    return ptr, col.astype(np.int32), w, ncols
