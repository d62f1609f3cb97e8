"""Runoff routing on the host (include/elmk.h "runoff routing"; the linear-reservoir river transport model of the CLM family, RTM), in
numpy only: the restatement of the stage the device performs (k_routing.hip), with the same operation order, and the host-side
helpers a driver needs.

    down = d8_network(nlat, nlon, direction)                            # or the driver's own network
    S.set_output_grid(ptr, col, w); S.water_balance_enable(tol)
    S.routing_enable(down, ddist, area, effvel=0.35, nsub=4)
    S.routing_init(volr_from_restart, qout_sum_from_restart, ncalls)    # or nothing: a cold start is all zeros
    ... the step ...; S.water_balance(dt); S.routing(dt)                # or S.run(dt, steps, st.RUN_ROUTING | st.RUN_WATER_BALANCE | ...)
    volr, qout = S.routing_read(VOLR), S.routing_read(QOUT)
    mean_discharge = S.routing_read(QOUT_SUM) / S.routing_count()

    qin = qin_from_rows(ptr, col, w, qrunoff, area)
    volr, qout = call(volr, qin, effvel / ddist, upstream_map(down), dt, nsub)
"""
import numpy as np

from . import diagnostics, regrid

VOLR, QIN, QOUT, QOUT_SUM = range(4)  # ELMK_ROUTE_*
MAXUP = 8
EFFVEL = 0.35  # RTM's effective velocity, m/s
_NAN = float(np.float64(np.nan))

# the refusals of elmk_routing_enable's network check (elmk_maps.h: route_check), in its order
E_NCELLS = "ncells outside 1 .. 2^31-1"
E_RANGE = "down outside [-1, ncells)"
E_SELF = "down equals its own index"
E_DEGREE = "more than 8 upstream cells drain into one cell"
E_CYCLE = "the network has a cycle"
E_DDIST = "ddist not finite and > 0"
E_AREA = "area not finite and >= 0"


def _canon(x):
    """A NaN is stored as the canonical quiet NaN."""
    return np.where(x != x, _NAN, x)


def check_network(down, ddist=None, area=None):
    """The checks of elmk_routing_enable on the network, in its order; raises ValueError with the entry point's text.  The cycle check
    follows every unvisited cell downstream with a three-colour mark (0 unvisited, 1 on the current path, 2 done), as the host does."""
    down = np.asarray(down).reshape(-1)
    n = down.size
    if n < 1 or n > 2 ** 31 - 1:
        raise ValueError(E_NCELLS)
    idx = np.arange(n)
    bad = (down < -1) | (down >= n) | (down == idx)
    if bad.any():
        c = int(np.nonzero(bad)[0][0])
        raise ValueError(E_RANGE if (down[c] < -1 or down[c] >= n) else E_SELF)
    if np.bincount(down[down >= 0], minlength=n).max(initial=0) > MAXUP:
        raise ValueError(E_DEGREE)
    mark = np.zeros(n, np.int8)
    dn = down.tolist()
    for c in range(n):
        if mark[c]:
            continue
        j = c
        while j >= 0 and mark[j] == 0:
            mark[j] = 1
            j = dn[j]
        if j >= 0 and mark[j] == 1:
            raise ValueError(E_CYCLE)
        j = c
        while j >= 0 and mark[j] == 1:
            mark[j] = 2
            j = dn[j]
    if ddist is not None:
        d = np.asarray(ddist, dtype=np.float64).reshape(-1)
        if d.size != n or not np.all(np.isfinite(d) & (d > 0.0)):
            raise ValueError(E_DDIST)
    if area is not None:
        a = np.asarray(area, dtype=np.float64).reshape(-1)
        if a.size != n or not np.all(np.isfinite(a) & (a >= 0.0)):
            raise ValueError(E_AREA)


def upstream_map(down):
    """up int32 [8, ncells]: row p holds, for cell c, the p-th cell u with down[u] == c in ascending u, else -1."""
    down = np.asarray(down).reshape(-1)
    n = down.size
    up = np.full((MAXUP, n), -1, np.int32)
    src = np.nonzero(down >= 0)[0]
    order = src[np.argsort(down[src], kind="stable")]  # by downstream cell, ascending u inside one
    dst = down[order]
    first = np.searchsorted(dst, dst, side="left")
    slot = np.arange(order.size) - first
    if slot.size and slot.max() >= MAXUP:
        raise ValueError(E_DEGREE)
    up[slot, dst] = order
    return up


def npad_of(up):
    """The rows of the map the device keeps: the largest in-degree rounded up to 1, 2, 4 or 8 (elmk_maps.h: ell_npad)."""
    nup = int((np.asarray(up) >= 0).sum(axis=0).max(initial=0))
    return 1 if nup <= 1 else 2 if nup <= 2 else 4 if nup <= 4 else 8


def flow(v, k, dts):
    """R2: v > 0: min-by-select of v * k and v / dts; anything else (NaN, zeros, negative) releases +0.0."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = v * k
        b = v / dts
        return np.where(v > 0.0, np.where(a < b, a, b), 0.0)


def call(volr, qin, kout, up, dt, nsub, in_place=False, cap=True):
    """One elmk_routing on the host: R0, R2 - R5.  volr, qin, kout: float64 [ncells]; up: upstream_map(down).  Returns (volr_new, qout).
    in_place and cap are the wrong variants the host tests hold their checks against: in_place updates the cells one after another in
    index order, each reading what the cells before it have already written; cap=False takes every flow without the cap v / dts,
    cap="own" only the upstream flows of R3."""
    v = np.array(volr, dtype=np.float64).reshape(-1)
    qin = np.asarray(qin, dtype=np.float64).reshape(-1)
    kout = np.asarray(kout, dtype=np.float64).reshape(-1)
    up = np.asarray(up)
    nsub = int(nsub)
    dts = float(dt) / float(nsub)
    qacc = np.zeros_like(v)
    safe = np.where(up >= 0, up, 0)

    def fl(x, k, own=True):
        if cap is True or (cap == "own" and own):
            return flow(x, k, dts)
        with np.errstate(all="ignore"):
            return np.where(x > 0.0, x * k, 0.0)

    with np.errstate(all="ignore"):
        for _ in range(nsub):
            if in_place:
                f = np.zeros_like(v)
                for c in range(v.size):
                    f[c] = fl(v[c], kout[c])
                    fin = 0.0
                    for p in range(up.shape[0]):
                        u = up[p, c]
                        if u >= 0:
                            fin = fin + float(fl(v[u], kout[u], False))
                    v[c] = v[c] + ((fin - f[c]) + qin[c]) * dts
            else:
                f = fl(v, kout)
                fu = f if cap != "own" else fl(v, kout, False)  # (flow(v_old[u], KOUT[u]) is cell u's own f: the same bits)
                fin = np.zeros_like(v)
                for p in range(up.shape[0]):
                    fin = np.where(up[p] >= 0, fin + fu[safe[p]], fin)
                v = _canon(v + ((fin - f) + qin) * dts)
            qacc = qacc + f
        qout = _canon(qacc / float(nsub))
    return _canon(v), qout


def qin_from_rows(ptr, col, w, qrunoff, area, qflx_irrig=None):
    """R1: QIN [ncells] from the column row QRUNOFF (mm/s) through the output grid's CSR map, regrid.apply_aggregate's arithmetic with
    +0.0 for a cell without terms; qflx_irrig: the withdrawal's column row, aggregated the same way and subtracted."""
    with np.errstate(all="ignore"):
        r = regrid.apply_aggregate(ptr, col, w, qrunoff, 0.0)
        if qflx_irrig is not None:
            r = r - regrid.apply_aggregate(ptr, col, w, qflx_irrig, 0.0)
        return _canon((r * 0.001) * np.asarray(area, dtype=np.float64).reshape(-1))


def budget(volr, qin, qout, down):
    """R6: the sums of VOLR and QIN and the sum of QOUT over the outlets, in the device reduction's order."""
    outlet = np.where(np.asarray(down).reshape(-1) < 0, np.asarray(qout, dtype=np.float64).reshape(-1), 0.0)
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (volr, qin, outlet)])


# D8 direction codes (the ESRI convention): the neighbour a cell drains into, as (row step, column step) with row 0 the northernmost
D8 = {1: (0, 1), 2: (1, 1), 4: (1, 0), 8: (1, -1), 16: (0, -1), 32: (-1, -1), 64: (-1, 0), 128: (-1, 1)}


def d8_network(nlat, nlon, direction):
    """down int32 [nlat * nlon] (row-major) from D8 direction codes [nlat, nlon]: 1 E, 2 SE, 4 S, 8 SW, 16 W, 32 NW, 64 N, 128 NE; any
    other code, and a direction that leaves the grid, makes the cell an outlet.  The result is checked (check_network)."""
    d = np.asarray(direction).reshape(nlat, nlon)
    i, j = np.indices((nlat, nlon))
    down = np.full((nlat, nlon), -1, np.int64)
    for code, (di, dj) in D8.items():
        m = d == code
        ti, tj = i + di, j + dj
        ok = m & (ti >= 0) & (ti < nlat) & (tj >= 0) & (tj < nlon)
        down[ok] = (ti * nlon + tj)[ok]
    down = down.reshape(-1).astype(np.int32)
    check_network(down)
    return down
