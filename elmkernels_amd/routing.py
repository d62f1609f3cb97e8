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

Its floodplain inundation (include/elmk.h "floodplain inundation"; k_kinematic_step's flood form), after S.routing_kinematic_enable:

    S.routing_inundation_enable(rdepth, eprof)                          # bank height [ncells], elevation profile [11, ncells]
    S.routing_inundation_init(wf_from_restart)
    ... S.routing(dt) and S.run(..., RUN_ROUTING) now spill over the banks and back ...
    wf, frac = S.routing_read(WF), S.routing_read(FLOOD_FRAC)

    tab = inundation_tables(area, params, rdepth, eprof)
    wh, wt, volr, qout, wf, depth, frac = kinematic_call(wh, wt, volr, qin, qsur, area, params, up, dt, nsub, flood=(tab, wf))

Its reservoirs (include/elmk.h "reservoirs"; the DAM form of both kernels), after S.routing_kinematic_enable:

    target, beta, mstart = reservoir_targets(mean_inflow, mean_demand, cap)   # or the driver's own
    S.routing_reservoir_enable(cap, target, beta, mstart)
    S.routing_reservoir_init(res_from_restart, krls_from_restart)
    S.routing_reservoir_time(month_of_doy(doy), month_begins(doy, decday)); S.routing(dt)   # S.run(..., RUN_ROUTING) derives the time
    res, take = S.routing_read(RES), S.routing_read(RES_TAKE)

    dam = {"tab": reservoir_tables(cap, target, beta, mstart), "res": res, "krls": krls, "month": m, "begins": b}
    wh, wt, volr, qout, res, krls, take, qin = kinematic_call(wh, wt, volr, qin, qsur, area, params, up, dt, nsub, dam=dam)

Its command areas (include/elmk.h "command areas"; k_kinematic_prep_cmd, k_command_allot, k_command_take), after
S.routing_reservoir_enable and S.routing_set_withdrawal(True):

    S.routing_command_enable(dam, share, claim)                         # [4, ncells] each: check_command says what they must hold
    ... S.routing(dt) and S.run(..., RUN_ROUTING) now let the dams supply the cells that hang on them ...
    take, give = S.routing_read(CMD_TAKE), S.routing_read(CMD_GIVE)

    dam["command"] = command_tables(cap, dam_rows, share, claim)
    ..., res, krls, take, qin, cmd_want, cmd_take, cmd_give, cmd_ratio = kinematic_call(..., dam=dam)

Its stream temperature (include/elmk.h "stream temperature"; the HEAT form of both kernels), after S.routing_kinematic_enable and
without the two extensions above:

    S.routing_heat_enable(sublev=2, shade=shade)
    S.routing_heat_init(tt_from_restart, tr_from_restart)
    ... S.routing(dt) and S.run(..., RUN_ROUTING) now carry TT and TR ...
    tt, tr = S.routing_read(TT), S.routing_read(TR)

    tab = heat_tables(params, sublev, shade)
    heat = {"tab": tab, "prep": heat_prep(ptr, col, w, columns, tab), "tt": tt, "tr": tr}
    wh, wt, volr, qout, tt, tr, heat_end, hin, hsrf, hadj, hout = kinematic_call(wh, wt, volr, qin, qsur, area, params, up, dt, nsub, heat=heat)
"""
import math

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


def land_from_rows(ptr, col, w, qflx_h2orof_drain):
    """F5's t [ncells]: the column row QFLX_H2OROF_DRAIN (mm/s) through the output grid's CSR map, regrid.apply_aggregate's arithmetic with
    +0.0 for a cell without terms - what kinematic_call takes as `land`."""
    with np.errstate(all="ignore"):
        return regrid.apply_aggregate(ptr, col, w, qflx_h2orof_drain, 0.0)


def kinematic_call(wh, wt, volr, qin, qsur, area, params, up, dt, nsub, in_place=False, cap=True, flood=None, dam=None, heat=None,
                   land=None):
    """One elmk_routing with the scheme on, on the host: K0, K2 - K7.  wh, wt, volr, qin, qsur, area: float64 [ncells]; params
    [11, ncells]; up: upstream_map(down).  Returns (wh_new, wt_new, volr_new, qout).  in_place and cap are the wrong variants the host
    tests hold their checks against, as call's: in_place updates the cells one after another in index order, the upstream flows taken
    from main-channel storages already updated in the sub-step; cap=False takes every flow without the cap v / dts.
    flood=(tables, wf): the flood form ("floodplain inundation", I1 - I6) with inundation_tables' tables and the floodplain storage wf
    [ncells]; returns (wh_new, wt_new, volr_new, qout, wf_new, flood_depth, flood_frac).
    dam: the DAM form ("reservoirs", D0 - D5), a dict with "tab" (reservoir_tables), "res" and "krls" [ncells], "month" (0 .. 11) and
    "begins"; optional "withdrawal" = (rn, i), R1's aggregates of QRUNOFF and QFLX_IRRIG [ncells] (the routing's withdrawal is on: D2;
    qin is then K1's QIN with the withdrawal), and "variant", one of the wrong variants of DAM_VARIANTS.  The result grows by
    (res_new, krls_new, res_take, qin_new) behind the flood rows, if any.  "command": the command areas ("command areas", C1 - C3;
    needs "withdrawal"), a dict of command_tables' entries plus optionally "take", "give" and "ratio" [ncells], the rows as the device
    holds them (the cells C0 leaves alone keep them; None: 0.0, 0.0 and 1.0), "variant", one of CMD_VARIANTS, and "census" (command_allot);
    C1 - C3 run after the first regulation and before the first sub-step's use of QSUB, qin_new is the credited QIN, and the result
    grows by (want, take, give, ratio) behind it.
    heat: the HEAT form ("stream temperature", H1 - H6), a dict with "tab" (heat_tables), "prep" (heat_prep), "tt" and "tr" [ncells] and
    optionally "census", a dict that takes a bool row per branch of HEAT_BRANCHES; not together with flood or dam.  The result grows by
    (tt_new, tr_new, heat, hin, hsrf, hadj, hout); the water rows keep their bits (H8).
    land: the LAND form of the K1 launch ("floodplain infiltration", F5), land_from_rows' aggregate of the column row
    QFLX_H2OROF_DRAIN [ncells]; only with flood.  QLAND = (land * 0.001) * area leaves wf before the first sub-step, and the result
    grows by (qland,) at its end."""
    if land is not None and (flood is None or heat is not None):
        raise ValueError("kinematic_call: land without flood, or with heat")
    if heat is not None:
        if flood is not None or dam is not None or in_place:
            raise ValueError("kinematic_call: heat with flood, dam or in_place")
    if dam is not None:
        if in_place:
            raise ValueError("kinematic_call: dam with in_place")
        dtab, dvar = dam["tab"], dam.get("variant")
        if dvar is not None and dvar not in DAM_VARIANTS:
            raise ValueError(f"kinematic_call: unknown variant {dvar!r}")
        res, krls, take, qin = reservoir_prep(dam["res"], dam["krls"], qin, area, dtab, dam["month"], dam["begins"], dt,
                                              dam.get("withdrawal"), d1_last=dvar == "d1_after_d2")
        dmonth = int(dam["month"])
        dkw = {"spill": dvar != "no_spill", "smin": dvar != "no_smin"}
        cmd = dam.get("command")
        if cmd is not None:
            if dam.get("withdrawal") is None:
                raise ValueError("kinematic_call: command areas without the withdrawal")
            cvar = cmd.get("variant")
            if cvar is not None and cvar not in CMD_VARIANTS:
                raise ValueError(f"kinematic_call: unknown variant {cvar!r}")
            with np.errstate(all="ignore"):  # C1: what R1 and D2 left of the withdrawal
                iv = (np.asarray(dam["withdrawal"][1], dtype=np.float64).reshape(-1) * 0.001) * np.asarray(area, dtype=np.float64).reshape(-1)
                cwant = command_want(np.where(dtab["DAM"], iv - take / float(dt), iv), dt, cmd)
            cres0 = np.asarray(dam["res"], dtype=np.float64).reshape(-1)
            ctake, cgive, cratio = (np.array(cmd[k], dtype=np.float64).reshape(-1) if cmd.get(k) is not None else None for k in ("take", "give", "ratio"))
    else:
        cmd = None
    if flood is not None:
        tab, wf = flood
        wf = np.array(wf, dtype=np.float64).reshape(-1)
        depth = frac = np.zeros_like(wf)
    wh, wt, v = (np.array(x, dtype=np.float64).reshape(-1) for x in (wh, wt, volr))
    qin, qsur, area = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (qin, qsur, area))
    p = np.asarray(params, dtype=np.float64)
    ch, ct, cr = kinematic_params(p)
    up = np.asarray(up)
    nsub = int(nsub)
    dts = float(dt) / float(nsub)
    qacc = np.zeros_like(v)
    safe = np.where(up >= 0, up, 0)
    ht = _HeatCall(heat, v.size) if heat is not None else None
    with np.errstate(all="ignore"):
        if land is not None:  # F5
            qland = _canon((np.asarray(land, dtype=np.float64).reshape(-1) * 0.001) * area)
            wf = _canon(wf - qland * float(dt))
        qsub = qin - qsur
        for sub in range(nsub):
            eh = hillslope_flow(wh, area, ch, dts, cap)
            et = channel_flow(wt, p[TLEN], p[TWIDTH], ct, dts, cap)
            er = channel_flow(v, p[RLEN], p[RWIDTH], cr, dts, cap)
            en = er  # K6's own term: the natural flow
            if dam is not None:  # D3 where K4 forms the flow of the coming sub-step: the same operands as forming it here; D4
                er, res = reservoir_regulate(en, res, krls, dtab, dmonth, dts, **dkw)
                if dvar == "own_eo":
                    en = er
                if cmd is not None and sub == 0:  # C2, C3: after the K1 launch's regulation, before the first sub-step's QSUB
                    res, cgive, cratio = command_allot(cwant, res, dtab, cmd, cgive, cratio, variant=cvar, res_avail=cres0,
                                                       census=cmd.get("census"))
                    ctake, qin, qsub = command_take(cwant, cratio, qin, qsur, dt, cmd, ctake, variant=cvar)
            if ht is not None:
                ht.before(wt, v, qsub, eh, et, er, up, safe, dts)
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
                v = _canon(v + ((fin - en) + et) * dts)
            if flood is not None:  # I1: after K6, before the next sub-step's er
                v, wf, depth, frac = inundation_exchange(v, wf, tab, area)
            wh = _canon(wh + (qsur - eh) * dts)
            wt = _canon(wt + ((eh - et) + qsub) * dts)
            if ht is not None:
                ht.after(wt, v, dts)
            qacc = qacc + er
        qout = _canon(qacc / float(nsub))
        if dam is not None and dvar == "regulate_last":
            res = reservoir_regulate(channel_flow(v, p[RLEN], p[RWIDTH], cr, dts, cap), res, krls, dtab, dmonth, dts, **dkw)[1]
    out = (wh, wt, _canon(v), qout)
    if flood is not None:
        out += (wf, depth, frac)
    if dam is not None:
        out += (res, krls, take, qin)
        if cmd is not None:
            out += (cwant, ctake, cgive, cratio)
    if ht is not None:
        out += ht.rows()
    if land is not None:
        out += (qland,)
    return out


def kinematic_budget(wh, wt):
    """K8: the sums of WH and WT in the device reduction's order."""
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (wh, wt)])


# ---- floodplain inundation (include/elmk.h "floodplain inundation", I0 - I8) -----------------------------------------------------------
WF, FLOOD_DEPTH, FLOOD_FRAC = 7, 8, 9  # ELMK_ROUTE_*, readable while the extension is on
NPROF = 11  # ELMK_FP_NPROF: the elevations of the profile, at the area fractions 0, 0.1 .. 1

# the refusals of elmk_routing_inundation_enable's check (elmk_maps.h: inundation_check), in its order; each is followed by the cell
E_RDEPTH = "RDEPTH not finite and > 0"
E_EPROF_FINITE = "EPROF not finite"
E_EPROF_ZERO = "EPROF[0] not 0"
E_EPROF_ORDER = "EPROF not increasing"


def e_cell(text, cell):
    """The refusal `text` as the entry point gives it: with the first offending cell."""
    return f"{text} at cell {cell}"


def check_inundation(rdepth, eprof):
    """The checks of elmk_routing_inundation_enable on rdepth [ncells] and eprof [11, ncells], in its order: rdepth cell by cell, then
    per cell the profile (finite, eprof[0] == 0.0, strictly increasing); raises ValueError with the entry point's text."""
    r = np.asarray(rdepth, dtype=np.float64).reshape(-1)
    e = np.asarray(eprof, dtype=np.float64)
    if e.ndim != 2 or e.shape != (NPROF, r.size):
        raise ValueError("eprof must be [11, ncells]")
    bad = ~(np.isfinite(r) & (r > 0.0))
    if bad.any():
        raise ValueError(e_cell(E_RDEPTH, int(np.nonzero(bad)[0][0])))
    with np.errstate(all="ignore"):
        code = np.where(~np.isfinite(e).all(axis=0), 1, np.where(~(e[0] == 0.0), 2, np.where(~(e[1:] > e[:-1]).all(axis=0), 3, 0)))
    if code.any():
        c = int(np.nonzero(code)[0][0])
        raise ValueError(e_cell((E_EPROF_FINITE, E_EPROF_ZERO, E_EPROF_ORDER)[int(code[c]) - 1], c))


def inundation_tables(area, params, rdepth, eprof):
    """I0: the checked inputs' tables, a dict of float64 arrays: ACHN, VC, AF [ncells]; E, S, VB [11, ncells]; DE, M [10, ncells]; F [11]
    (f_k).  area [ncells], params [11, ncells] as kinematic_call's (RLEN and RWIDTH are read)."""
    check_inundation(rdepth, eprof)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    p = np.asarray(params, dtype=np.float64)
    e = np.array(eprof, dtype=np.float64)
    with np.errstate(all="ignore"):
        achn = p[RLEN] * p[RWIDTH]
        vc = achn * np.asarray(rdepth, dtype=np.float64).reshape(-1)
        af = area - achn
        af = np.where(af > 0.0, af, 0.0)
        f = np.arange(NPROF, dtype=np.float64) / 10.0
        s = achn[None] + af[None] * f[:, None]
        de = e[1:] - e[:-1]
        m = (af * 0.1)[None] / de
        vb = np.zeros_like(e)
        for k in range(NPROF - 1):
            vb[k + 1] = vb[k] + (0.5 * (s[k] + s[k + 1])) * de[k]
    return {"ACHN": achn, "VC": vc, "AF": af, "E": e, "F": f, "S": s, "DE": de, "M": m, "VB": vb}


def inundation_exchange(volr, wf, tab, area):
    """I1 - I4 for every cell: volr, the main channel's storage K6 has just formed, and wf, the floodplain's, brought to one water
    level.  Returns (volr_new, wf_new, flood_depth, flood_frac); a cell that I1 leaves untouched keeps its bits."""
    v = np.asarray(volr, dtype=np.float64).reshape(-1)
    wf = np.asarray(wf, dtype=np.float64).reshape(-1)
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    vc, achn, af, e, f, s, de, m, vb = (tab[k] for k in ("VC", "ACHN", "AF", "E", "F", "S", "DE", "M", "VB"))
    with np.errstate(all="ignore"):
        touched = (wf > 0.0) | (v > vc)  # I1
        w = v + wf
        over = touched & (w > vc)  # I3, I4; touched & ~over: I2
        x = w - vc
        top = x >= vb[10]
        k = np.zeros(v.size, np.int64)
        for j in range(1, NPROF - 1):
            k = np.where(x >= vb[j], j, k)

        def at(t):
            return np.take_along_axis(t, k[None], axis=0)[0]

        r = x - at(vb)
        sk, mk, dek = at(s), at(m), at(de)
        d = (2.0 * r) / (sk + np.sqrt(sk * sk + (2.0 * mk) * r))
        d = np.where(d > dek, dek, d)
        h = np.where(top, e[10] + (x - vb[10]) / s[10], at(e) + d)
        fr = np.where(top, 1.0, f[k] + (0.1 * d) / dek)
        vc2 = vc + achn * h
        vc2 = np.where(vc2 > w, w, vc2)
        frac = np.where(area > 0.0, (af * fr) / np.where(area > 0.0, area, 1.0), 0.0)
        v_new = np.where(over, vc2, np.where(touched, w, v))
        wf_new = np.where(touched, _canon(np.where(over, w - vc2, 0.0)), wf)  # (an untouched WF is not stored)
        return _canon(v_new), wf_new,_canon(np.where(over, h, 0.0)), _canon(np.where(over, frac, 0.0))


def inundation_budget(wf):
    """I7: the sum of WF in the device reduction's order, float64 [1]."""
    return np.array([diagnostics.reduce_min_max_sum(wf)[2]])


QLAND = 20  # ELMK_ROUTE_QLAND, readable while the floodplain infiltration is on


def land_budget(qland):
    """F6: the sum of QLAND in the device reduction's order, float64 [1]."""
    return np.array([diagnostics.reduce_min_max_sum(qland)[2]])


# ---- reservoirs (include/elmk.h "reservoirs", D0 - D8) -----------------------------------------------------------------------------------
RES, KRLS, RES_TAKE = 10, 11, 12  # ELMK_ROUTE_*, readable while the extension is on
NMONTH = 12
MONTH_FIRST_DOY = (0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334)  # the no-leap calendar
DAM_VARIANTS = ("own_eo", "regulate_last", "no_spill", "no_smin", "d1_after_d2")  # the wrong variants the host tests hold the statement against
DAM_BRANCHES = ("floored", "fill", "draw unlimited", "draw limited", "pass-through", "spill", "beta < 1", "take limited", "take unlimited")

# the refusals of elmk_routing_reservoir_enable's check (elmk_maps.h: reservoir_check), in its order; each is followed by the cell
E_CAP = "CAP not finite and >= 0"
E_TARGET = "TARGET not finite and >= 0"
E_BETA = "BETA outside [0, 1]"
E_MSTART = "MSTART outside 0 .. 11"


def check_reservoirs(cap, target, beta, mstart):
    """The checks of elmk_routing_reservoir_enable on cap [ncells], target [12, ncells], beta [ncells] and mstart [ncells], in its
    order: cap cell by cell, then per dam cell (cap > 0) target, beta, mstart; raises ValueError with the entry point's text."""
    c = np.asarray(cap, dtype=np.float64).reshape(-1)
    t = np.asarray(target, dtype=np.float64)
    b = np.asarray(beta, dtype=np.float64).reshape(-1)
    m = np.asarray(mstart).reshape(-1)
    if t.ndim != 2 or t.shape != (NMONTH, c.size) or b.size != c.size or m.size != c.size:
        raise ValueError("target must be [12, ncells], beta and mstart [ncells]")
    bad = ~(np.isfinite(c) & (c >= 0.0))
    if bad.any():
        raise ValueError(e_cell(E_CAP, int(np.nonzero(bad)[0][0])))
    with np.errstate(all="ignore"):
        code = np.where(~(np.isfinite(t) & (t >= 0.0)).all(axis=0), 1, np.where(~((b >= 0.0) & (b <= 1.0)), 2, np.where((m < 0) | (m > 11), 3, 0)))
    code = np.where(c > 0.0, code, 0)
    if code.any():
        k = int(np.nonzero(code)[0][0])
        raise ValueError(e_cell((E_TARGET, E_BETA, E_MSTART)[int(code[k]) - 1], k))


def reservoir_tables(cap, target, beta, mstart):
    """The checked inputs' tables as the host derives them, a dict: CAP, SMIN = 0.1 * CAP, C85 = 0.85 * CAP, BETA [ncells], TARGET
    [12, ncells], MSTART int32 [ncells], DAM bool [ncells] (D0); the rows of cells without a dam are 0."""
    check_reservoirs(cap, target, beta, mstart)
    c = np.asarray(cap, dtype=np.float64).reshape(-1)
    dam = c > 0.0
    c = np.where(dam, c, 0.0)
    return {"CAP": c, "SMIN": 0.1 * c, "C85": 0.85 * c, "BETA": np.where(dam, np.asarray(beta, dtype=np.float64).reshape(-1), 0.0),
            "TARGET": np.where(dam[None], np.asarray(target, dtype=np.float64), 0.0),
            "MSTART": np.where(dam, np.asarray(mstart).reshape(-1), 0).astype(np.int32), "DAM": dam}


def month_of_doy(doy):
    """The month 0 .. 11 of day-of-year doy (0 = 1 January) in the no-leap calendar; any other doy is taken modulo 365."""
    return int(np.searchsorted(MONTH_FIRST_DOY, int(doy) % 365, side="right")) - 1


def month_begins(doy, decday):
    """Whether a step with (doy, decday) starts at 00:00 of the first day of its month: the active layer's rollover test,
    decday == doy + 1.0, on the first doy of each month."""
    return 0 <= int(doy) <= 364 and int(doy) in MONTH_FIRST_DOY and float(decday) == float(int(doy)) + 1.0


def reservoir_prep(res, krls, qin, area, tab, month, begins, dt, withdrawal=None, d1_last=False, census=None):
    """D1 and D2, the K1 launch's part for the dam cells: res, krls, qin (K1's QIN), area [ncells]; withdrawal = (rn, i), R1's
    aggregates of QRUNOFF and QFLX_IRRIG, or None while the routing's withdrawal is off.  Returns (res, krls, res_take, qin).
    d1_last: D1 after D2 (a wrong variant).  census: a dict that takes the bool rows "take limited" and "take unlimited"."""
    res, krls = (np.array(x, dtype=np.float64).reshape(-1) for x in (res, krls))
    qin, area = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (qin, area))
    dam = tab["DAM"]
    take = np.zeros_like(res)
    with np.errstate(all="ignore"):
        def d1(res, krls):
            on = dam & bool(begins) & (int(month) == tab["MSTART"])
            return np.where(on, _canon(res / np.where(on, tab["C85"], 1.0)), krls)

        if not d1_last:
            krls = d1(res, krls)
        if withdrawal is not None:
            rn, i = (np.asarray(x, dtype=np.float64).reshape(-1) for x in withdrawal)
            iv = (i * 0.001) * area
            want = iv * dt
            a = res - tab["SMIN"]
            avail = np.where(a > 0.0, a, 0.0)
            limited = want > avail
            t = np.where(limited, avail, want)
            res = np.where(dam, _canon(res - t), res)
            take = np.where(dam, _canon(t), 0.0)
            qin = np.where(dam, _canon((rn * 0.001) * area - (iv - t / dt)), qin)
            if census is not None:
                census["take limited"] = dam & limited
                census["take unlimited"] = dam & ~limited & (want > 0.0)
        if d1_last:
            krls = d1(res, krls)
    return res, krls, take, qin


def reservoir_regulate(e, res, krls, tab, month, dts, spill=True, smin=True, census=None):
    """D3 for every cell: e, the main channel's er that K4 has just formed, res and krls [ncells].  Returns (eo, res_new); a cell without
    a dam keeps e and its res.  spill=False and smin=False are wrong variants (no spill over CAP; no dead storage).  census: a dict
    that takes a bool row per branch of DAM_BRANCHES[:7]."""
    e, res, krls = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (e, res, krls))
    dam, cap, beta = tab["DAM"], tab["CAP"], tab["BETA"]
    sm = tab["SMIN"] if smin else np.zeros_like(cap)
    tgt = tab["TARGET"][int(month)]
    with np.errstate(all="ignore"):
        q = beta * (krls * tgt) + (1.0 - beta) * e
        qmin = 0.1 * e
        floored = q < qmin
        q = np.where(floored, qmin, q)
        draw = q > e
        a = res - sm
        x = q - e
        lim = np.where(a > 0.0, a / dts, 0.0)
        limited = x > lim
        x = np.where(limited, lim, x)
        eo = np.where(draw, e + x, q)
        s = res + (e - eo) * dts
        over = (s > cap) if spill else np.zeros(s.shape, bool)
        eo = np.where(over, eo + (s - cap) / dts, eo)
        s = np.where(over, cap, s)
    if census is not None:
        census.update({"floored": dam & floored, "fill": dam & ~draw & (q < e), "draw unlimited": dam & draw & ~limited,
                       "draw limited": dam & draw & limited & (a > 0.0), "pass-through": dam & draw & ~(a > 0.0), "spill": dam & over,
                       "beta < 1": dam & (beta < 1.0)})
    return np.where(dam, _canon(eo), e), np.where(dam, _canon(s), res)


def reservoir_budget(res, res_take):
    """D6: the sums of RES and RES_TAKE in the device reduction's order."""
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (res, res_take)])


def reservoir_targets(mean_inflow, mean_demand, cap):
    """TARGET, BETA and MSTART from a climatology, by the rules of Hanasaki et al. (2006): mean_inflow and mean_demand [12] or
    [12, ncells], the mean monthly inflow and irrigation demand in m3/s; cap [ncells] or a scalar, m3.  With im and dm the annual means
    of the two (the mean over the twelve months):
      TARGET[m] = im                                  where dm == 0 (a dam that serves no irrigation),
                = (im / 2) * (1 + demand[m] / dm)     where dm >= 0.5 * im,
                = im + demand[m] - dm                 otherwise (never below 0);
      c = cap / (im * 365 * 86400), the storage as a share of the annual inflow volume;  BETA = min(1, (c / 0.5) ** 2);
      MSTART = the first month with inflow < im that follows a month with inflow >= im (the operational year begins when the inflow
               falls below its mean; 0 where no month does).
    Returns (target float64 [12, ncells], beta float64 [ncells], mstart int32 [ncells]).
    With the command areas on (check_command) a dam also supplies the cells that depend on it: mean_demand should then include the
    command area's demand - the dependents' mean withdrawal times their share - beside the own cell's."""
    cap = np.atleast_1d(np.asarray(cap, dtype=np.float64)).reshape(-1)
    fi = np.asarray(mean_inflow, dtype=np.float64)
    fd = np.asarray(mean_demand, dtype=np.float64)
    fi = np.repeat(fi[:, None], cap.size, axis=1) if fi.ndim == 1 else fi
    fd = np.repeat(fd[:, None], cap.size, axis=1) if fd.ndim == 1 else fd
    if fi.shape != (NMONTH, cap.size) or fd.shape != (NMONTH, cap.size):
        raise ValueError("mean_inflow and mean_demand must be [12] or [12, ncells]")
    im, dm = fi.mean(axis=0), fd.mean(axis=0)
    with np.errstate(all="ignore"):
        share = (im[None] / 2.0) * (1.0 + fd / np.where(dm > 0.0, dm, 1.0)[None])
        shift = np.maximum(im[None] + fd - dm[None], 0.0)
        target = np.where((dm == 0.0)[None], np.repeat(im[None], NMONTH, axis=0), np.where((dm >= 0.5 * im)[None], share, shift))
        c = cap / np.where(im > 0.0, im * (365.0 * 86400.0), 1.0)
        beta = np.where(im > 0.0, np.minimum(1.0, (c / 0.5) ** 2), 1.0)
    below = fi < im[None]
    falls = below & ~np.roll(below, 1, axis=0)
    mstart = np.where(falls.any(axis=0), falls.argmax(axis=0), 0).astype(np.int32)
    return target, beta, mstart


# ---- command areas (include/elmk.h "command areas", C0 - C8) ------------------------------------------------------------------------------
CMD_WANT, CMD_TAKE, CMD_GIVE, CMD_RATIO = 21, 22, 23, 24  # ELMK_ROUTE_CMD_*, readable while the part is on
NDEP = 4  # ELMK_CMD_NDEP: the slots of a cell's dependency rows
CMD_VARIANTS = ("reverse", "ratio_on_want", "no_smin", "before_d2", "no_credit")  # the wrong variants the host tests hold the statement against

# the refusals of elmk_routing_command_enable's check (elmk_maps.h: command_check), in its order; each is followed by the cell
E_CMD_RANGE = "DAM outside [-1, ncells)"
E_CMD_GAP = "DAM filled behind an empty slot"
E_CMD_NODAM = "DAM names a cell without a reservoir"
E_CMD_SELF = "DAM names the cell itself"
E_CMD_TWICE = "DAM names one reservoir twice"
E_CMD_SHARE = "SHARE outside (0, 1]"
E_CMD_CLAIM = "CLAIM outside [0, 1]"
E_CMD_SHARE_SUM = "SHARE sums to more than 1"
E_CMD_CLAIM_SUM = "CLAIM sums to more than 1"  # followed by the dam's cell


def _command_terms(cap, dam):
    """The inverse map of checked rows: (dams, ptr, cell, slot) - the dam list (every cell with cap > 0, ascending), the CSR over it, and
    the terms (cell, slot) sorted by cell and then slot.  A counting sort: linear time."""
    n = cap.size
    dams = np.nonzero(cap > 0.0)[0]
    place = np.full(n, -1, np.int64)
    place[dams] = np.arange(dams.size)
    cell = np.repeat(np.arange(n)[:, None], NDEP, axis=1).reshape(-1)  # cell-major, slot-minor: sorted by cell and then slot
    slot = np.tile(np.arange(NDEP), n)
    d = dam.T.reshape(-1)
    filled = d >= 0
    cell, slot, d = cell[filled], slot[filled], d[filled]
    order = np.argsort(place[d], kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(place[d], minlength=dams.size))]).astype(np.int64)
    return dams.astype(np.int32), ptr, cell[order].astype(np.int32), slot[order].astype(np.int32)


def check_command(cap, dam, share, claim):
    """The checks of elmk_routing_command_enable on cap [ncells] (the reservoirs' CAP) and the rows dam (int), share and claim
    [4, ncells], in its order: per cell in index order and per slot in slot order the index, the gap, the reservoir, the cell itself,
    the repeat, share, claim; behind a cell's slots its shares added in slot order; then per dam in ascending order its claims added
    in term order.  Raises ValueError with the entry point's text."""
    cap = np.asarray(cap, dtype=np.float64).reshape(-1)
    dam, share, claim = np.asarray(dam), np.asarray(share, dtype=np.float64), np.asarray(claim, dtype=np.float64)
    n = cap.size
    if dam.shape != (NDEP, n) or share.shape != dam.shape or claim.shape != dam.shape:
        raise ValueError("dam, share and claim must be [4, ncells]")
    dam = dam.astype(np.int64)
    code = np.zeros((NDEP, n), np.int64)  # per slot the first failing check, 0: none
    filled = dam >= 0
    safe = np.where(filled & (dam < n), dam, 0)
    gap = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for k in range(NDEP):
            twice = np.zeros(n, bool)
            for j in range(k):
                twice |= dam[j] == dam[k]
            c = np.where((dam[k] < -1) | (dam[k] >= n), 1,
                np.where(~filled[k], 0,
                np.where(gap, 2,
                np.where(~(cap[safe[k]] > 0.0), 3,
                np.where(dam[k] == np.arange(n), 4,
                np.where(twice, 5,
                np.where(~(np.isfinite(share[k]) & (share[k] > 0.0) & (share[k] <= 1.0)), 6,
                np.where(~((claim[k] >= 0.0) & (claim[k] <= 1.0)), 7, 0))))))))
            code[k] = c
            gap |= ~filled[k]
        first = np.where(code.any(axis=0), np.take_along_axis(code, (code != 0).argmax(axis=0)[None], axis=0)[0], 0)
        # the shares' sum is checked behind a cell's slots: only in a cell whose slots all pass
        ok = filled & (code == 0)
        total = np.zeros(n)
        for k in range(NDEP):
            total = np.where(ok[k], share[k] if k == 0 else total + share[k], total)
        first = np.where((first == 0) & ~(total <= 1.0), 8, first)
    if first.any():
        c = int(np.nonzero(first)[0][0])
        raise ValueError(e_cell((E_CMD_RANGE, E_CMD_GAP, E_CMD_NODAM, E_CMD_SELF, E_CMD_TWICE, E_CMD_SHARE, E_CMD_CLAIM, E_CMD_SHARE_SUM)[int(first[c]) - 1], c))
    dams, ptr, cell, slot = _command_terms(cap, dam)
    q = claim[slot, cell]
    for j in range(dams.size):
        total = 0.0
        for p in range(int(ptr[j]), int(ptr[j + 1])):
            total = float(q[p]) if p == ptr[j] else total + float(q[p])
        if not total <= 1.0:
            raise ValueError(e_cell(E_CMD_CLAIM_SUM, int(dams[j])))


def command_tables(cap, dam, share, claim):
    """The checked rows' tables as the host derives them, a dict: DAM int32 [4, ncells] (-1 in every empty slot), SHARE and CLAIM
    float64 [4, ncells] (0.0 there), HAS bool [ncells] (a filled slot 0), and the inverse map "dams" [ndams], "ptr" [ndams + 1], "cell",
    "slot" and "share" [nterms] in CSR order."""
    check_command(cap, dam, share, claim)
    cap = np.asarray(cap, dtype=np.float64).reshape(-1)
    d = np.asarray(dam).astype(np.int32)
    filled = d >= 0
    dams, ptr, cell, slot = _command_terms(cap, d)
    s = np.where(filled, np.asarray(share, dtype=np.float64), 0.0)
    return {"DAM": np.where(filled, d, -1).astype(np.int32), "SHARE": s, "CLAIM": np.where(filled, np.asarray(claim, dtype=np.float64), 0.0),
            "HAS": filled[0], "dams": dams, "ptr": ptr, "cell": cell, "slot": slot, "share": s[slot, cell]}


def command_want(rest, dt, cmd):
    """C1: WANT [ncells] from rest, what R1 and D2 left of the cells' withdrawal in m3/s; 0.0 in a cell without a filled slot."""
    rest = np.asarray(rest, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        return np.where(cmd["HAS"] & (rest > 0.0), rest * float(dt), 0.0)


def command_allot(want, res, tab, cmd, give=None, ratio=None, variant=None, res_avail=None, census=None):
    """C2 for every dam with terms: want [ncells] (C1), res [ncells] as the K1 launch left it, tab: reservoir_tables, cmd:
    command_tables.  Returns (res_new, give, ratio); a dam without terms keeps its res and the give and ratio handed in (None: 0.0 and
    1.0).  variant: "reverse" adds a dam's terms last to first, "no_smin" forms avail without SMIN, "before_d2" forms avail from
    res_avail, the RES before D2's take (wrong variants).  census: a dict that takes bool rows over the cells, "limited", "unlimited"
    (W > 0), "W = 0", "no terms" and "at or below SMIN"."""
    want, res = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (want, res))
    n = res.size
    give = np.zeros(n) if give is None else np.array(give, dtype=np.float64).reshape(-1)
    ratio = np.ones(n) if ratio is None else np.array(ratio, dtype=np.float64).reshape(-1)
    dams, ptr = cmd["dams"].astype(np.int64), cmd["ptr"]
    nd = dams.size
    cnt = np.diff(ptr)
    with np.errstate(all="ignore"):
        x = cmd["share"] * want[cmd["cell"]]
        W = np.zeros(nd)
        for k in range(int(cnt.max(initial=0))):  # the k-th term of every dam that has one, in CSR order (reverse: from the last)
            on = cnt > k
            p = np.where(on, (ptr[1:] - 1 - k) if variant == "reverse" else (ptr[:-1] + k), 0)
            xk = x[p] if x.size else np.zeros(nd)
            W = np.where(on, xk if k == 0 else W + xk, W)
        base = np.asarray(res_avail, dtype=np.float64).reshape(-1) if variant == "before_d2" else res
        a = base[dams] - (0.0 if variant == "no_smin" else tab["SMIN"][dams])
        avail = np.where(a > 0.0, a, 0.0)
        limited = W > avail
        r = np.where(limited, avail / np.where(limited, W, 1.0), 1.0)
        G = W * r
        has = cnt > 0
        res_new, give, ratio = res.copy(), give, ratio
        res_new[dams[has]] = _canon(res[dams] - G)[has]
        give[dams[has]] = _canon(G)[has]
        ratio[dams[has]] = _canon(r)[has]
    if census is not None:
        def row(mask):
            out = np.zeros(n, bool)
            out[dams[mask]] = True
            return out
        census.update({"limited": row(has & limited), "unlimited": row(has & ~limited & (W > 0.0)), "W = 0": row(has & (W == 0.0)),
                       "no terms": row(~has), "at or below SMIN": row(has & ~(a > 0.0))})
    return res_new, give, ratio


def command_take(want, ratio, qin, qsur, dt, cmd, take=None, variant=None):
    """C3 for every cell with a filled slot: want (C1), ratio (C2's row), qin and qsur [ncells].  Returns (take, qin_new, qsub_new); a
    cell without a filled slot keeps the take handed in (None: 0.0) and its qin.  variant: "ratio_on_want" forms share * (WANT * RATIO),
    "no_credit" leaves QIN as it is (wrong variants)."""
    want, ratio, qin, qsur = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (want, ratio, qin, qsur))
    take = np.zeros(want.size) if take is None else np.asarray(take, dtype=np.float64).reshape(-1)
    dam, has = cmd["DAM"], cmd["HAS"]
    with np.errstate(all="ignore"):
        got = np.zeros(want.size)
        for k in range(NDEP):
            on = dam[k] >= 0
            rk = ratio[np.where(on, dam[k], 0)]
            x = cmd["SHARE"][k] * (want * rk) if variant == "ratio_on_want" else (cmd["SHARE"][k] * want) * rk
            got = np.where(on, x if k == 0 else got + x, got)
        q = qin if variant == "no_credit" else _canon(qin + got / float(dt))
        qin_new = np.where(has, q, qin)
        return np.where(has, _canon(got), take), qin_new, qin_new - qsur


def command_budget(give, take):
    """C5: the sums of CMD_GIVE and CMD_TAKE in the device reduction's order."""
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (give, take)])


# ---- stream temperature (include/elmk.h "stream temperature", H0 - H9) -------------------------------------------------------------------
TT, TR, HEAT, HIN, HSRF, HADJ, HOUT = range(13, 20)  # ELMK_ROUTE_*, readable while the extension is on
TFRZ, TMAX, RHOCP, EMIS, SB, ALBW, CPAIR, LV, RAIR, CEX, DMIN = 273.15, 313.15, 4188000.0, 0.97, 5.67e-8, 0.1, 1004.64, 2.501e6, 287.04, 1.3e-3, 1e-3
NSUBLEV = 15
HEAT_PREP_ROWS = ("RAD", "KE", "EMS", "TA", "QA", "PA", "TSUR", "TSUB")
HEAT_BRANCHES = ("terms", "no terms", "QSUB > 0", "QSUB <= 0", "WT > WMINT", "WT <= WMINT", "VOLR > WMINR", "VOLR <= WMINR",
                 "settle inside", "settle TFRZ", "settle TMAX", "settle TEQ")

# the refusals of elmk_routing_heat_enable's check (elmk_maps.h: heat_check), in its order; E_SHADE is followed by the cell
E_SUBLEV = "sublev outside 0 .. 14"
E_SHADE = "SHADE outside [0, 1]"


def _exp1(v):
    try:
        return math.exp(v)
    except OverflowError:  # (glibc returns +inf and raises the overflow flag)
        return float("inf")


def _vexp(x):
    """exp per element through math.exp (glibc's bits, which the device's elmk_exp restates; np.exp is not guaranteed to give them),
    +inf where glibc overflows."""
    x = np.asarray(x, dtype=np.float64)
    return np.fromiter((_exp1(v) for v in x.reshape(-1).tolist()), np.float64, x.size).reshape(x.shape)


def _fl(t):
    """fl(t) = t > TFRZ ? t : TFRZ: a NaN gives TFRZ."""
    return np.where(np.asarray(t, dtype=np.float64) > TFRZ, t, TFRZ)


def check_heat(sublev, shade=None, ncells=None):
    """The checks of elmk_routing_heat_enable on sublev and shade [ncells] (None: 0.0 everywhere), in its order; raises ValueError with
    the entry point's text."""
    if not 0 <= int(sublev) < NSUBLEV:
        raise ValueError(E_SUBLEV)
    if shade is None:
        return
    s = np.asarray(shade, dtype=np.float64).reshape(-1)
    if ncells is not None and s.size != ncells:
        raise ValueError("shade must be [ncells]")
    with np.errstate(all="ignore"):
        bad = ~((s >= 0.0) & (s <= 1.0))
    if bad.any():
        raise ValueError(e_cell(E_SHADE, int(np.nonzero(bad)[0][0])))


def heat_tables(params, sublev=0, shade=None):
    """H0: the checked inputs' tables, a dict: AT, ACHN, WMINT, WMINR, KSW float64 [ncells], EMS0 and "sublev".  params [11, ncells] as
    kinematic_call's (TLEN, TWIDTH, RLEN and RWIDTH are read)."""
    p = np.asarray(params, dtype=np.float64)
    check_heat(sublev, shade, p.shape[1])
    s = np.zeros(p.shape[1]) if shade is None else np.asarray(shade, dtype=np.float64).reshape(-1)
    at, achn = p[TLEN] * p[TWIDTH], p[RLEN] * p[RWIDTH]
    return {"AT": at, "ACHN": achn, "WMINT": at * DMIN, "WMINR": achn * DMIN, "KSW": (1.0 - ALBW) * (1.0 - s), "EMS0": (EMIS * SB) / RHOCP,
            "sublev": int(sublev)}


def heat_prep(ptr, col, w, cols, tab):
    """H1's aggregates and derived rows: a dict of float64 [ncells] over HEAT_PREP_ROWS plus "TEQ" and "terms" (bool).  cols: the column
    fields as the device stores them, widened - forc_tbot, forc_pbot, forc_qbot, forc_lwrad, forc_u, forc_v, t_grnd [ncols]; forc_solad,
    forc_solai [ncols, 2]; t_soisno [ncols, 20] - through the output grid's CSR map, regrid.apply_aggregate's arithmetic."""
    def f(k):
        return np.asarray(cols[k], dtype=np.float64)

    def agg(x):
        return regrid.apply_aggregate(ptr, col, w, x, 0.0)

    ptr = np.asarray(ptr)
    terms = ptr[1:] > ptr[:-1]
    with np.errstate(all="ignore"):
        ta, pa, qa, lw = agg(f("forc_tbot")), agg(f("forc_pbot")), agg(f("forc_qbot")), agg(f("forc_lwrad"))
        ua = agg(np.sqrt(f("forc_u") * f("forc_u") + f("forc_v") * f("forc_v")))
        sd, si = f("forc_solad"), f("forc_solai")
        sw = agg(((sd[:, 0] + sd[:, 1]) + si[:, 0]) + si[:, 1])
        tsur, tsub = agg(_fl(f("t_grnd"))), agg(_fl(f("t_soisno")[:, 5 + tab["sublev"]]))
        rad = (tab["KSW"] * sw + EMIS * lw) / RHOCP
        ke = ((pa / (RAIR * ta)) * CEX) * ua
        out = {"RAD": np.where(terms, rad, 0.0), "KE": np.where(terms, ke, 0.0), "EMS": np.where(terms, tab["EMS0"], 0.0),
               "TA": np.where(terms, ta, 0.0), "QA": np.where(terms, qa, 0.0), "PA": np.where(terms, pa, 0.0),
               "TSUR": np.where(terms, tsur, TFRZ), "TSUB": np.where(terms, tsub, TFRZ)}
    out = {k: _canon(v) for k, v in out.items()}
    out["TEQ"] = _fl(out["TA"])
    out["terms"] = terms
    return out


def heat_phi(t, x):
    """H2: phi(T) [ncells], K m/s, with x heat_prep's rows."""
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = t - TFRZ
        es = 611.2 * _vexp((17.67 * d) / (t - 29.65))
        qs = (0.622 * es) / (x["PA"] - 0.378 * es)
        t2 = t * t
        return (x["RAD"] - x["EMS"] * (t2 * t2)) + (x["KE"] * (CPAIR * (x["TA"] - t) - LV * (qs - x["QA"]))) / RHOCP


def heat_settle(h, wn, wmin, teq, census=None):
    """H5: (t, adj) [ncells].  census: a dict whose bool rows "settle inside", "settle TFRZ", "settle TMAX" and "settle TEQ" take the
    cells of each outcome (or-ed in)."""
    with np.errstate(all="ignore"):
        held = wn > wmin
        t0 = h / np.where(held, wn, 1.0)
        low = ~(t0 >= TFRZ)
        t1 = np.where(low, TFRZ, t0)
        high = t1 > TMAX
        t = np.where(held, np.where(high, TMAX, t1), teq)
        adj = np.where(held & ~low & ~high, 0.0, t * wn - h)
    if census is not None:
        for k, v in (("settle inside", held & ~low & ~high), ("settle TFRZ", held & low), ("settle TMAX", held & high), ("settle TEQ", ~held)):
            census[k] = census.get(k, False) | v
    return t, adj


def heat_budget(heat, hin, hsrf, hadj, hout, down):
    """H7: the sums of HEAT, HIN, HSRF and HADJ and the sum of HOUT over the outlets, in the device reduction's order."""
    outlet = np.where(np.asarray(down).reshape(-1) < 0, np.asarray(hout, dtype=np.float64).reshape(-1), 0.0)
    return np.array([diagnostics.reduce_min_max_sum(x)[2] for x in (heat, hin, hsrf, hadj, outlet)])


class _HeatCall:
    """H3 - H6 inside kinematic_call: the state of the call's heat and its two hooks, before and after a sub-step's water."""

    def __init__(self, heat, n):
        self.tab, self.x, self.census = heat["tab"], heat["prep"], heat.get("census")
        self.tt, self.tr = (np.array(heat[k], dtype=np.float64).reshape(-1) for k in ("tt", "tr"))
        self.hin, self.hsrf, self.hadj, self.hout, self.heat = (np.zeros(n) for _ in range(5))
        self.mag = heat.get("mag")  # a list that takes, per sub-step, the sum of the magnitudes of every term the cell's heat handled

    def before(self, wt, v, qsub, eh, et, er, up, safe, dts):
        tab, x, tt, tr = self.tab, self.x, self.tt, self.tr
        hr = _canon(er * tr)
        fh = np.zeros_like(v)
        for k in range(up.shape[0]):
            fh = np.where(up[k] >= 0, fh + hr[safe[k]], fh)
        gb = np.where(qsub > 0.0, qsub * x["TSUB"], qsub * tt)  # H3
        wet_t, wet_r = wt > tab["WMINT"], v > tab["WMINR"]
        self.sxt = np.where(wet_t, tab["AT"] * heat_phi(tt, x), 0.0)
        self.hi = eh * x["TSUR"] + gb
        self.h_t = tt * wt + ((self.hi - et * tt) + self.sxt) * dts
        self.sxr = np.where(wet_r, tab["ACHN"] * heat_phi(tr, x), 0.0)  # H4
        self.ho = hr
        self.h_r = tr * v + (((fh - hr) + et * tt) + self.sxr) * dts
        if self.mag is not None:
            fa = np.zeros_like(v)
            for k in range(up.shape[0]):
                fa = np.where(up[k] >= 0, fa + np.abs(hr[safe[k]]), fa)
            self._m = (np.abs(tt * wt) + np.abs(tr * v) +
                       (np.abs(eh * x["TSUR"]) + np.abs(gb) + 2.0 * np.abs(et * tt) + np.abs(self.sxt) + np.abs(self.sxr) + fa + np.abs(hr)) * dts)
        if self.census is not None:
            for k, m in (("terms", x["terms"]), ("no terms", ~x["terms"]), ("QSUB > 0", qsub > 0.0), ("QSUB <= 0", ~(qsub > 0.0)),
                         ("WT > WMINT", wet_t), ("WT <= WMINT", ~wet_t), ("VOLR > WMINR", wet_r), ("VOLR <= WMINR", ~wet_r)):
                self.census[k] = self.census.get(k, False) | m

    def after(self, wtn, vn, dts):
        tab, teq = self.tab, self.x["TEQ"]
        ttn, adjt = heat_settle(self.h_t, wtn, tab["WMINT"], teq, self.census)
        trn, adjr = heat_settle(self.h_r, vn, tab["WMINR"], teq, self.census)
        self.tt, self.tr = _canon(ttn), _canon(trn)
        self.hin = _canon(self.hin + self.hi * dts)  # H6
        self.hsrf = _canon(self.hsrf + (self.sxt + self.sxr) * dts)
        self.hadj = _canon(self.hadj + (adjt + adjr))
        self.hout = _canon(self.hout + self.ho * dts)
        self.heat = _canon(ttn * wtn + trn * vn)
        if self.mag is not None:
            self.mag.append(self._m + np.abs(ttn * wtn) + np.abs(trn * vn) + np.abs(adjt) + np.abs(adjr) + np.abs(self.hin) + np.abs(self.hsrf) +
                            np.abs(self.hadj) + np.abs(self.hout))

    def rows(self):
        return self.tt, self.tr, self.heat, self.hin, self.hsrf, self.hadj, self.hout


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
