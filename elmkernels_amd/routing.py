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

The kinematic-wave scheme (include/elmk.h "kinematic-wave routing"; k_kinematic_prep, k_kinematic_step), after S.soil_hydrology_enable:

    S.routing_kinematic_enable(params)                                  # [11, ncells]: HSLP .. NR
    S.routing_kinematic_init(wh_from_restart, wt_from_restart)
    ... S.routing(dt) and S.run(..., RUN_ROUTING) now route through hillslope, tributaries and main channel ...
    wh, wt = S.routing_read(WH), S.routing_read(WT)

    qsur = qsur_from_rows(ptr, col, w, qflx_surf, qflx_h2osfc_surf, area)
    wh, wt, volr, qout = kinematic_call(wh, wt, volr, qin, qsur, area, params, upstream_map(down), dt, nsub)
"""
import numpy as np

from . import diagnostics, regrid
from .hydrology import _pow

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


# ---- kinematic-wave routing (include/elmk.h "kinematic-wave routing", K0 - K9) ---------------------------------------------------------
WH, WT, QSUR = 4, 5, 6  # ELMK_ROUTE_*, readable while the scheme is on
HSLP, NH, GXR, TLEN, TWIDTH, TSLP, NT, RLEN, RWIDTH, RSLP, NR = range(11)  # ELMK_KW_*: the rows of the parameters
NPARAM = 11
PARAM_NAMES = ("HSLP", "NH", "GXR", "TLEN", "TWIDTH", "TSLP", "NT", "RLEN", "RWIDTH", "RSLP", "NR")
T23, T53 = 2.0 / 3.0, 5.0 / 3.0


def e_param(row):
    """The refusal of elmk_routing_kinematic_enable's parameter check (elmk_maps.h: kinematic_check) for row `row`."""
    return PARAM_NAMES[row] + " not finite and > 0"


def kinematic_params(params):
    """The check of elmk_routing_kinematic_enable on params [11, ncells] (every value finite and > 0; raises ValueError with the entry
    point's text, which names the first failing row) and the host's derivation: returns (CH, CT, CR) with
    CH = (sqrt(HSLP) / NH) * GXR, CT = sqrt(TSLP) / NT, CR = sqrt(RSLP) / NR."""
    p = np.asarray(params, dtype=np.float64)
    if p.ndim != 2 or p.shape[0] != NPARAM:
        raise ValueError("params must be [11, ncells]")
    for k in range(NPARAM):
        if not np.all(np.isfinite(p[k]) & (p[k] > 0.0)):
            raise ValueError(e_param(k))
    return (np.sqrt(p[HSLP]) / p[NH]) * p[GXR], np.sqrt(p[TSLP]) / p[NT], np.sqrt(p[RSLP]) / p[NR]


def _vpow(x, y):
    """pow per element through math.pow (glibc's bits; np.power is not guaranteed to give them), with hydrology._pow's handling of
    its exceptions."""
    x = np.asarray(x, dtype=np.float64)
    return np.fromiter((_pow(v, y) for v in x.reshape(-1).tolist()), np.float64, x.size).reshape(x.shape)


def _cap(v, a, dts, cap=True):
    """K2: v > 0: min-by-select of the rate a and v / dts; anything else releases +0.0.  cap=False: the rate alone (a wrong variant)."""
    with np.errstate(all="ignore"):
        if cap:
            b = v / dts
            a = np.where(a < b, a, b)
        return np.where(v > 0.0, a, 0.0)


def hillslope_flow(wh, area, ch, dts, cap=True):
    """K3: eh [ncells].  The rate is formed only where it is taken (wh > 0 and area > 0); elsewhere the flow is +0.0 (K9)."""
    wh = np.asarray(wh, dtype=np.float64)
    area = np.asarray(area, dtype=np.float64)
    on = (wh > 0.0) & (area > 0.0)
    with np.errstate(all="ignore"):
        h = np.where(on, wh, 1.0) / np.where(on, area, 1.0)
        a = (ch * _vpow(h, T53)) * area
        return np.where(on, _cap(wh, a, dts, cap), 0.0)


def channel_flow(w, length, width, c, dts, cap=True):
    """K4: chan(w, len, wid, c) [ncells], the tributaries' et and the main channel's er."""
    w = np.asarray(w, dtype=np.float64)
    on = w > 0.0
    with np.errstate(all="ignore"):
        a = np.where(on, w, 1.0) / length
        y = a / width
        p = width + 2.0 * y
        r = a / p
        q = (c * _vpow(r, T23)) * a
        return np.where(on, _cap(w, q, dts, cap), 0.0)


def qsur_from_rows(ptr, col, w, qflx_surf, qflx_h2osfc_surf, area):
    """K1: QSUR [ncells] from the soil hydrology's column rows QFLX_SURF and QFLX_H2OSFC_SURF (mm/s), aggregated as qin_from_rows does."""
    with np.errstate(all="ignore"):
        x = np.asarray(qflx_surf, dtype=np.float64) + np.asarray(qflx_h2osfc_surf, dtype=np.float64)
        s = regrid.apply_aggregate(ptr, col, w, x, 0.0)
        return _canon((s * 0.001) * np.asarray(area, dtype=np.float64).reshape(-1))


def kinematic_call(wh, wt, volr, qin, qsur, area, params, up, dt, nsub, in_place=False, cap=True):
    """One elmk_routing with the scheme on, on the host: K0, K2 - K7.  wh, wt, volr, qin, qsur, area: float64 [ncells]; params
    [11, ncells]; up: upstream_map(down).  Returns (wh_new, wt_new, volr_new, qout).  in_place and cap are the wrong variants the host
    tests hold their checks against, as call's: in_place updates the cells one after another in index order, the upstream flows taken
    from main-channel storages already updated in the sub-step; cap=False takes every flow without the cap v / dts."""
    wh, wt, v = (np.array(x, dtype=np.float64).reshape(-1) for x in (wh, wt, volr))
    qin, qsur, area = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (qin, qsur, area))
    p = np.asarray(params, dtype=np.float64)
    ch, ct, cr = kinematic_params(p)
    up = np.asarray(up)
    nsub = int(nsub)
    dts = float(dt) / float(nsub)
    qacc = np.zeros_like(v)
    safe = np.where(up >= 0, up, 0)
    with np.errstate(all="ignore"):
        qsub = qin - qsur
        for _ in range(nsub):
            eh = hillslope_flow(wh, area, ch, dts, cap)
            et = channel_flow(wt, p[TLEN], p[TWIDTH], ct, dts, cap)
            er = channel_flow(v, p[RLEN], p[RWIDTH], cr, dts, cap)
            if in_place:
                for c in range(v.size):
                    fin = 0.0
                    for k in range(up.shape[0]):
                        u = up[k, c]
                        if u >= 0:
                            fin = fin + float(channel_flow(v[u:u + 1], p[RLEN, u], p[RWIDTH, u], cr[u], dts, cap)[0])
                    v[c] = v[c] + ((fin - er[c]) + et[c]) * dts
            else:
                fin = np.zeros_like(v)
                for k in range(up.shape[0]):
                    fin = np.where(up[k] >= 0, fin + er[safe[k]], fin)
                v = _canon(v + ((fin - er) + et) * dts)
            wh = _canon(wh + (qsur - eh) * dts)
            wt = _canon(wt + ((eh - et) + qsub) * dts)
            qacc = qacc + er
        qout = _canon(qacc / float(nsub))
    return wh, wt, _canon(v), qout


def kinematic_budget(wh, wt):
    """K8: the sums of WH and WT in the device reduction's order."""
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (wh, wt)])


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
