"""Column soil hydrology on the host (include/elmk.h "soil hydrology"; ELM v1's SoilHydrologyMod in the CLM4.5 formulation): the
restatement of the stage the device performs (k_soil_hydrology.hip), one column at a time in plain Python floats, so that every
operation is one IEEE fp64 operation in the order of the header and nothing is fused.  The reference has no soil hydrology; the header's
text is the specification and `step` is its host truth.

    S.soil_hydrology_enable()
    S.soil_hydrology_set_params(hksat_from_texture(...), wtfact, h2osfc_thresh(sigma), k_wet(slope), rsub_top_max(slope))
    S.soil_hydrology_init()                         # ELM's cold start: wa = 4000 mm, zwt = cold_start_zwt(zisoi)
    advance_physics(S, dt); S.soil_hydrology(dt)    # or S.run(dt, steps, RUN_HYDROLOGY)
    S.soil_hydrology_frost_enable(q_perch_max(slope))   # optional: the frost table and the perched water table (the header's F');
                                                        # step(..., frost=rows) is that form on the host
    S.hillslope_enable(down, dist, width, area, elev, k_aniso)  # optional: lateral flow along hillslopes (the header's L1 - L3);
                                                                # step(..., lat=(down, dist, width, area, elev, k_aniso)) on the host

pow, exp and erf are math.pow / math.exp / math.erf per element (glibc), which the device's elmk_pow / elmk_exp restate bit for bit;
np.power and np.exp are not guaranteed to.  min(a, b) and max(a, b) are (b < a ? b : a) and (a < b ? b : a), written out.
"""
import math

import numpy as np

NLEVSNO = 5
N = 10  # hydrologically active soil layers: layer j is level 5 + j of h2osoi_liq, h2osoi_ice, dz, zsoi; its bottom level 6 + j of zisoi
DENH2O, DENICE, E_ICE, SMPMIN, WATMIN = 1000.0, 917.0, 6.0, -1.0e8, 0.01
PC, MU, FFF_S, FFF_D, AQUIFER_MAX, ROUS_MIN = 0.4, 0.13889, 0.5, 2.5, 5000.0, 0.02
WA_COLD = 4000.0
TFRZ, SAT_LEV = 273.15, 0.9  # F': the frost table and the perched water table

# the rows of the feature (ELMK_HYD_*)
ZWT, WA, HKSAT, WTFACT, H2OSFC_THRESH, K_WET, RSUB_TOP_MAX = 0, 1, 2, 12, 13, 14, 15
QFLX_SURF, QFLX_INFL, QFLX_H2OSFC_SURF, QFLX_DRAIN, QFLX_RSUB_SAT, QCHARGE, FSAT = range(16, 23)
NROWS = 23
# the rows of the frost-table extension (ELMK_HYDF_*)
Q_PERCH_MAX, FROST_TABLE, ZWT_PERCHED, QFLX_DRAIN_PERCHED = range(4)
FROST_NROWS = 4
DIAGNOSTICS = ("qflx_surf", "qflx_infl", "qflx_h2osfc_surf", "qflx_drain", "qflx_rsub_sat", "qcharge", "fsat")

# the state fields the stage reads, and those it writes
READS = ("h2osoi_liq", "h2osoi_ice", "dz", "zsoi", "zisoi", "watsat", "sucsat", "bsw", "h2osfc", "frac_h2osfc", "frac_sno_eff", "snl",
         "qflx_top_soil", "qflx_rootsoi", "qflx_evap_grnd", "qflx_ev_soil", "qflx_ev_h2osfc", "qflx_dew_grnd", "qflx_dew_snow",
         "qflx_sub_snow")
WRITES = ("h2osoi_liq", "h2osoi_ice", "h2osoi_vol", "h2osfc")

_NAN = float(np.float64(np.nan))
_INF = float("inf")


def _min(a, b):
    return b if b < a else a


def _max(a, b):
    return b if a < b else a


def _div(a, b):
    """IEEE a / b (Python raises where IEEE gives an infinity or a NaN)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return _NAN
    return math.copysign(_INF, a) * math.copysign(1.0, b)


def _pow(x, y):
    try:
        return math.pow(x, y)
    except ValueError:
        return _NAN if x < 0.0 else _INF  # a negative base with a fractional exponent; 0 to a negative power
    except OverflowError:
        return _INF


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return _INF


def _canon(x):
    return _NAN if x != x else x


def cold_start_zwt(zi9):
    """ELM's cold start of the water table from the bottom of layer 9 (level 15 of zisoi): zi + 25 - wa / 0.2 / 1000 with wa = 4000 mm,
    that is zi + 5 m up to rounding."""
    return (zi9 + 25.0) - WA_COLD / 0.2 / 1000.0


def _sy(zwt, watsat, sucsat, bsw):
    return _max(ROUS_MIN, watsat * (1.0 - _pow(1.0 + _div(1.0e3 * zwt, sucsat), _div(-1.0, bsw))))


def _jwt(zwt, zi):
    for j in range(N):
        if zwt <= zi[j + 1]:
            return j
    return N


def _lat_rise(rt, zwt, jwt, liq, zi, watsat, sucsat, bsw):
    """L3's rising walk ("hillslope lateral flow"): E's with rt for qt and the water into every visited layer of liq (changed in place).
    Returns (what is left of rt, the water table, the layers visited, whether the walk ended inside a layer)."""
    for j in range(jwt, -1, -1):
        sy = _sy(zwt, watsat[j], sucsat[j], bsw[j])
        ql = _max(0.0, _min(rt, sy * (zwt - zi[j]) * 1.0e3))
        liq[j] = liq[j] + ql
        zwt = zwt - _div(_div(ql, sy), 1000.0)
        rt = rt - ql
        if rt <= 0.0:
            return rt, zwt, jwt - j + 1, True
    return rt, zwt, jwt + 1, False


def column(c, dt, hit=None, probe=None):
    """One column: c is a dict of Python floats / lists (see step); returns the dict of outputs.  hit: a set that collects the
    names of the branches taken (the tests assert coverage from it).  probe: a dict that receives copies of D's intermediates - the
    tridiagonal rows a, b, cc, r and the solution u (N + 1 each), the interface fluxes q and their derivatives dq1, dq2, the
    conductivities hk, the matric potentials smp (N each) and the equilibrium potentials zq (N + 1); and under "walks", per walk over
    the layers that ran (E_rise, E_fall, F_drain, FA_remove, FB_remove), (the layers it visited, whether it ran off the end of the
    layers with a remainder left)."""
    walks = {}

    def mark(name):
        if hit is not None:
            hit.add(name)

    liq, ice, dz, z = list(c["liq"]), list(c["ice"]), c["dz"], c["z"]
    zi = c["zi"]  # zi[0] = the surface, zi[j + 1] = the bottom of layer j
    watsat, sucsat, bsw, hksat, rootsoi = c["watsat"], c["sucsat"], c["bsw"], c["hksat"], c["rootsoi"]
    zwt, wa, h2osfc = c["zwt"], c["wa"], c["h2osfc"]
    frac_h2osfc, fsno, snl, top = c["frac_h2osfc"], c["fsno"], c["snl"], c["qflx_top_soil"]

    # A. ice and porosity
    effpor, icefrac, vol_liq, vol = [0.0] * N, [0.0] * N, [0.0] * N, [0.0] * N
    zmm, dzmm, zimm = [0.0] * (N + 1), [0.0] * (N + 1), [v * 1.0e3 for v in zi]
    for j in range(N):
        vol_ice = _min(watsat[j], _div(ice[j], dz[j] * DENICE))
        effpor[j] = _max(0.01, watsat[j] - vol_ice)
        icefrac[j] = _min(1.0, _div(vol_ice, watsat[j]))
        vol_liq[j] = _div(_max(liq[j], 1.0e-6), dz[j] * DENH2O)
        vol[j] = _div(liq[j], dz[j] * DENH2O) + _div(ice[j], dz[j] * DENICE)
        zmm[j] = z[j] * 1.0e3
        dzmm[j] = dz[j] * 1.0e3

    # B. surface runoff
    fsat = c["wtfact"] * _exp(-0.5 * FFF_S * zwt)
    qflx_surf = fsat * top

    # C. infiltration and h2osfc
    qevap = c["qflx_evap_grnd"] if snl == 0 else c["qflx_ev_soil"]
    q_in_soil = (1.0 - frac_h2osfc) * (top - qflx_surf)
    q_in_soil = q_in_soil - (1.0 - fsno - frac_h2osfc) * qevap
    q_in_sfc = frac_h2osfc * (top - qflx_surf)
    q_in_sfc = q_in_sfc - frac_h2osfc * c["qflx_ev_h2osfc"]
    m = _pow(10.0, -E_ICE * icefrac[0]) * hksat[0]
    m = _min(m, _pow(10.0, -E_ICE * icefrac[1]) * hksat[1])
    m = _min(m, _pow(10.0, -E_ICE * icefrac[2]) * hksat[2])
    qinmax = (1.0 - fsat) * m
    excess = _max(0.0, q_in_soil - (1.0 - frac_h2osfc) * qinmax)
    if excess > 0.0:
        mark("infiltration_excess")
    infl = q_in_soil - excess
    q_in_sfc = q_in_sfc + excess
    frac_infclust = 0.0 if frac_h2osfc <= PC else _pow(frac_h2osfc - PC, MU)
    thresh = c["h2osfc_thresh"]
    if h2osfc >= thresh:
        mark("h2osfc_above_threshold")
        qs = c["k_wet"] * frac_infclust * (h2osfc - thresh)
        qs = _min(qs, _div(h2osfc - thresh, dt))
    else:
        mark("h2osfc_below_threshold")
        qs = 0.0
    if qs < 1.0e-8:
        qs = 0.0
    else:
        mark("h2osfc_runoff")
    h2osfc = h2osfc + (q_in_sfc - qs) * dt
    if h2osfc < 0.0:
        mark("h2osfc_negative")
        infl = infl + _div(h2osfc, dt)
        h2osfc = 0.0
        drain_sfc = 0.0
    else:
        drain_sfc = _min(frac_h2osfc * qinmax, _div(h2osfc, dt))
    h2osfc = h2osfc - drain_sfc * dt
    infl = infl + drain_sfc
    rof = c.get("rof")
    if rof is not None:  # F1 - F3 ("floodplain infiltration"): rof = (in a cell, WF, FLOOD_FRAC, area of the cell)
        in_cell, wf, ff, ar = rof
        if in_cell and wf > 0.0 and ff > 0.0 and ar > 0.0:
            hr = _div(wf, ar) * 1000.0
            a, b = ff * qinmax, _div(hr, dt)
            d = a if a < b else b
            mark("rof_a" if a < b else "rof_b")
            fr = ff
        else:
            mark("rof_guard")
            hr = d = fr = 0.0
        infl = infl + d

    # D. soil water
    jwt = _jwt(zwt, zi)
    mark("jwt_0" if jwt == 0 else ("jwt_N" if jwt == N else "jwt_mid"))
    zwtmm = zwt * 1.0e3
    zq = [0.0] * (N + 1)
    for j in range(N):
        b1 = 1.0 - _div(1.0, bsw[j])
        if zwtmm <= zimm[j]:
            ve = watsat[j]
        elif zwtmm < zimm[j + 1]:
            t0 = _pow(_div(sucsat[j] + zwtmm - zimm[j], sucsat[j]), b1)
            v1 = _div(_div(-sucsat[j] * watsat[j], b1), zwtmm - zimm[j]) * (1.0 - t0)
            ve = _div(v1 * (zwtmm - zimm[j]) + watsat[j] * (zimm[j + 1] - zwtmm), zimm[j + 1] - zimm[j])
        else:
            ti = _pow(_div(sucsat[j] + zwtmm - zimm[j + 1], sucsat[j]), b1)
            t0 = _pow(_div(sucsat[j] + zwtmm - zimm[j], sucsat[j]), b1)
            ve = _div(_div(-sucsat[j] * watsat[j], b1), zimm[j + 1] - zimm[j]) * (ti - t0)
        ve = _min(watsat[j], _max(ve, 0.0))
        zq[j] = _max(SMPMIN, -sucsat[j] * _pow(_max(_div(ve, watsat[j]), 0.01), -bsw[j]))
    L = N - 1
    if jwt == N:
        b1 = 1.0 - _div(1.0, bsw[L])
        t0 = _pow(_div(sucsat[L] + zwtmm - zimm[N], sucsat[L]), b1)
        ve = _div(_div(-sucsat[L] * watsat[L], b1), zwtmm - zimm[N]) * (1.0 - t0)
        ve = _min(watsat[L], _max(ve, 0.0))
        zq[N] = _max(SMPMIN, -sucsat[L] * _pow(_max(_div(ve, watsat[L]), 0.01), -bsw[L]))
        zmm[N] = 0.5 * (zwtmm + zmm[L])
        dzmm[N] = zwtmm - zimm[N]
    hk, dhkdw, imped, smp, dsmpdw = [0.0] * N, [0.0] * N, [0.0] * N, [0.0] * N, [0.0] * N
    for j in range(N):
        jp = _min(N - 1, j + 1)
        s1 = _min(1.0, _div(0.5 * (vol[j] + vol[jp]), 0.5 * (watsat[j] + watsat[jp])))
        s2 = hksat[j] * _pow(s1, 2.0 * bsw[j] + 2.0)
        imped[j] = _pow(10.0, -E_ICE * (0.5 * (icefrac[j] + icefrac[jp])))
        if imped[j] < 1.0:
            mark("imped")
        hk[j] = imped[j] * s1 * s2
        dhkdw[j] = imped[j] * (2.0 * bsw[j] + 3.0) * s2 * _div(1.0, watsat[j] + watsat[jp])
        sn = _min(1.0, _max(_div(vol_liq[j], watsat[j]), 0.01))
        smp[j] = _max(SMPMIN, -sucsat[j] * _pow(sn, -bsw[j]))
        dsmpdw[j] = _div(-bsw[j] * smp[j], sn * watsat[j])
    # the interfaces: q[i] between nodes i and i + 1; interface N - 1 is towards the aquifer node
    q, dq1, dq2 = [0.0] * N, [0.0] * N, [0.0] * N
    for i in range(N - 1):
        den = zmm[i + 1] - zmm[i]
        num = (smp[i + 1] - smp[i]) - (zq[i + 1] - zq[i])
        q[i] = _div(-hk[i] * num, den)
        dq1[i] = _div(-(-hk[i] * dsmpdw[i] + num * dhkdw[i]), den)
        dq2[i] = _div(-(hk[i] * dsmpdw[i + 1] + num * dhkdw[i]), den)
    if jwt == N:
        sn1 = _min(1.0, _max(_div(vol[L], watsat[L]), 0.01))
        smp1 = _max(SMPMIN, -sucsat[L] * _pow(sn1, -bsw[L]))
        dsmpdw1 = _div(-bsw[L] * smp1, sn1 * watsat[L])
        den = zmm[N] - zmm[L]
        num = (smp1 - smp[L]) - (zq[N] - zq[L])
        q[L] = _div(-hk[L] * num, den)
        dq1[L] = _div(-(-hk[L] * dsmpdw[L] + num * dhkdw[L]), den)
        dq2[L] = _div(-(hk[L] * dsmpdw1 + num * dhkdw[L]), den)
    # the rows
    a, b, cc, r = [0.0] * (N + 1), [0.0] * (N + 1), [0.0] * (N + 1), [0.0] * (N + 1)
    r[0] = infl - q[0] - rootsoi[0]
    b[0] = _div(dzmm[0], dt) + dq1[0]
    cc[0] = dq2[0]
    for j in range(1, N):
        r[j] = q[j - 1] - q[j] - rootsoi[j]
        a[j] = -dq1[j - 1]
        b[j] = _div(dzmm[j], dt) - dq2[j - 1] + dq1[j]
        cc[j] = dq2[j]
    if jwt == N:
        r[N] = q[L]
        a[N] = -dq1[L]
        b[N] = _div(dzmm[N], dt) - dq2[L]
    else:
        b[N] = 1.0
    # the Thomas algorithm
    gam, u = [0.0] * (N + 1), [0.0] * (N + 1)
    bet = b[0]
    u[0] = _div(r[0], bet)
    for j in range(1, N + 1):
        gam[j] = _div(cc[j - 1], bet)
        bet = b[j] - a[j] * gam[j]
        u[j] = _div(r[j] - a[j] * u[j - 1], bet)
    for j in range(N - 1, -1, -1):
        u[j] = u[j] - gam[j + 1] * u[j + 1]
    if probe is not None:
        probe.update(a=list(a), b=list(b), cc=list(cc), r=list(r), u=list(u), q=list(q), dq1=list(dq1), dq2=list(dq2), hk=list(hk),
                     smp=list(smp), zq=list(zq), walks=walks)
    for j in range(N):
        liq[j] = liq[j] + u[j] * dzmm[j]
    # recharge
    if jwt == N:
        qcharge = _div(u[N] * dzmm[N], dt)
    else:
        k, up = jwt, _max(0, jwt - 1)
        sn = _max(_div(vol[k], watsat[k]), 0.01)
        ka = imped[k] * hksat[k] * _pow(_min(1.0, sn), 2.0 * bsw[k] + 3.0)
        wh = smp[up] - zq[up]
        if jwt == 0:
            qcharge = _div(-ka * (0.0 - wh), (zwt + 1.0e-3) * 1000.0)
        else:
            qcharge = _div(-ka * (0.0 - wh), (zwt - z[jwt - 1]) * 1000.0 * 2.0)
        qcharge = _max(_div(-10.0, dt), qcharge)
        qcharge = _min(_div(10.0, dt), qcharge)

    # E. water table
    if jwt == N:
        rous = _sy(zwt, watsat[L], sucsat[L], bsw[L])
        wa = wa + qcharge * dt
        zwt = zwt - _div(_div(qcharge * dt, 1000.0), rous)
    else:
        rous = _sy(zwt, watsat[L], sucsat[L], bsw[L])
        qt = qcharge * dt
        if qt > 0.0:
            mark("table_rises")
            walks["E_rise"] = (jwt + 1, True)
            for j in range(jwt, -1, -1):
                sy = _sy(zwt, watsat[j], sucsat[j], bsw[j])
                ql = _max(0.0, _min(qt, sy * (zwt - zi[j]) * 1.0e3))
                zwt = zwt - _div(_div(ql, sy), 1000.0)
                qt = qt - ql
                if qt <= 0.0:
                    walks["E_rise"] = (jwt - j + 1, False)
                    break
        else:
            mark("table_falls")
            walks["E_fall"] = (N - jwt, True)
            for j in range(jwt, N):
                sy = _sy(zwt, watsat[j], sucsat[j], bsw[j])
                ql = _min(0.0, _max(qt, -(sy * (zi[j + 1] - zwt) * 1.0e3)))
                qt = qt - ql
                if qt >= 0.0:
                    zwt = zwt - _div(_div(ql, sy), 1000.0)
                    walks["E_fall"] = (j - jwt + 1, False)
                    break
                zwt = zi[j + 1]
            if qt < 0.0:
                zwt = zwt - _div(_div(qt, 1000.0), rous)
    jwt = _jwt(zwt, zi)

    # F. drainage
    rous = _sy(zwt, watsat[L], sucsat[L], bsw[L])
    frost = "t" in c and "q_perch_max" in c
    above = False
    if frost:
        # F'. the frost table and the perched water table (replace F.1 and F.2)
        t, qpm = c["t"], c["q_perch_max"]

        def qsat(j0, j1):  # the thickness-weighted conductivity of layers j0 .. j1
            qs, ws = 0.0, 0.0
            for j in range(j0, j1 + 1):
                qs = qs + imped[j] * hksat[j] * dzmm[j]
                ws = ws + dzmm[j]
            if ws > 0.0:
                qs = _div(qs, ws)
            return qs

        def remove(rt, j0, j1, zw, walk):  # take -rt out of layers j0 .. j1 from the top; returns (what is left of rt, the table)
            walks[walk] = (j1 - j0 + 1, True)
            for j in range(j0, j1 + 1):
                rl = _max(rt, -(liq[j] - WATMIN))
                rl = _min(rl, 0.0)
                rt = rt - rl
                liq[j] = liq[j] + rl
                if rt >= 0.0:
                    zw = zw - _div(_div(rl, effpor[j]), 1000.0)
                    walks[walk] = (j - j0 + 1, False)
                    break
                zw = zi[j + 1]
            return rt, zw

        kf = N - 1 if t[0] > TFRZ else 0
        for k in range(1, N):
            if t[k - 1] > TFRZ and t[k] <= TFRZ:
                kf = k
                break
        ft = z[kf]
        frozen = t[kf] <= TFRZ
        zwp, qp = ft, 0.0
        if zwt < ft and frozen:
            mark("frost_A")
            above = True
            qp = qpm * qsat(jwt, kf) * (ft - zwt)
            rt, zwt = remove(-qp * dt, jwt, kf, zwt, "FA_remove")
            if rt < 0.0:
                mark("frost_A_exhausted")
            qp = qp + _div(rt, dt)
            rsub_top = 0.0
            jwt = _jwt(zwt, zi)
        else:
            def v(k):
                return _div(liq[k], dz[k] * DENH2O) + _div(ice[k], dz[k] * DENICE)

            kp = 0
            for k in range(kf, -1, -1):
                if _div(v(k), watsat[k]) <= SAT_LEV:
                    kp = k
                    break
            if not frozen:
                kp = kf
            if kf > kp:
                mark("frost_B_perched")
                s1, s2 = _div(v(kp), watsat[kp]), _div(v(kp + 1), watsat[kp + 1])
                m = _div(z[kp + 1] - z[kp], s2 - s1)
                b = z[kp + 1] - m * s2
                zwp = _max(0.0, m * SAT_LEV + b)
                qp = qpm * qsat(kp, kf) * (ft - zwp)
                rt, zwp = remove(-qp * dt, kp + 1, kf, zwp, "FB_remove")
                mark("perched_ends_in_layer" if rt >= 0.0 else "perched_exhausted")
                qp = qp + _div(rt, dt)
            else:
                mark("frost_B_none" if frozen else "frost_B_thawed")
    if not above:
        si, sd = 0.0, 0.0
        for j in range(_max(jwt - 1, 0), N):
            si = si + icefrac[j] * dzmm[j]
            sd = sd + dzmm[j]
        imp = _pow(10.0, -E_ICE * _div(si, sd))
        rsub_top = imp * c["rsub_top_max"] * _exp(-FFF_D * zwt)
        lat = c.get("lat")  # L3 ("hillslope lateral flow"): QLAT_NET of a column on a hillslope, in the place of the baseflow
        if lat is not None:
            rsub_top = lat
        rt = -rsub_top * dt
        if jwt == N:
            mark("drain_aquifer")
            if lat is not None:
                mark("lat_aquifer_inflow" if rt > 0.0 else "lat_aquifer")
            wa = wa + rt
            zwt = zwt - _div(_div(rt, 1000.0), rous)
            liq[L] = liq[L] + _max(0.0, wa - AQUIFER_MAX)
            wa = _min(wa, AQUIFER_MAX)
        elif lat is not None and rt > 0.0:
            rt, zwt, visited, ended = _lat_rise(rt, zwt, jwt, liq, zi, watsat, sucsat, bsw)
            walks["L_rise"] = (visited, not ended)
            mark("lat_rise_in_layer" if ended else "lat_rise_surface")
            liq[0] = liq[0] + rt
        else:
            if lat is not None:
                mark("lat_fall")
            mark("drain_soil")
            walks["F_drain"] = (N - jwt, True)
            for j in range(jwt, N):
                sy = _sy(zwt, watsat[j], sucsat[j], bsw[j])
                ql = _min(0.0, _max(rt, -(sy * (zi[j + 1] - zwt) * 1.0e3)))
                liq[j] = liq[j] + ql
                rt = rt - ql
                if rt >= 0.0:
                    zwt = zwt - _div(_div(ql, sy), 1000.0)
                    walks["F_drain"] = (j - jwt + 1, False)
                    break
                zwt = zi[j + 1]
            zwt = zwt - _div(_div(rt, 1000.0), rous)
            wa = wa + rt
    zwt = 0.0 if zwt < 0.0 else zwt
    zwt = 80.0 if 80.0 < zwt else zwt
    for j in range(N - 1, 0, -1):
        cap = effpor[j] * dzmm[j]
        xs = _max(liq[j] - cap, 0.0)
        if xs > 0.0:
            mark("excess_up")
        liq[j] = _min(cap, liq[j])
        liq[j - 1] = liq[j - 1] + xs
    xs1 = _max(_max(liq[0], 0.0) - _max(0.0, watsat[0] * dzmm[0] - ice[0]), 0.0)
    if xs1 > 0.0:
        mark("excess_to_h2osfc")
    liq[0] = liq[0] - xs1
    h2osfc = h2osfc + xs1
    rsub_sat = 0.0
    for j in range(N - 1):
        if liq[j] < WATMIN:
            mark("watmin_push_down")
            xs = WATMIN - liq[j]
            liq[j] = liq[j] + xs
            liq[j + 1] = liq[j + 1] - xs
    if liq[L] < WATMIN:
        mark("watmin_search")
        xs = WATMIN - liq[L]
        for i in range(N - 2, -1, -1):
            if xs > 0.0:
                avail = _max(liq[i] - WATMIN - xs, 0.0)
                take = _min(avail, xs)
                liq[L] = liq[L] + take
                liq[i] = liq[i] - take
                xs = _max(xs - take, 0.0)
        if xs > 0.0:
            mark("watmin_remainder")
        liq[L] = liq[L] + xs
        rsub_top = rsub_top - _div(xs, dt)
    qflx_drain = rsub_sat + rsub_top

    # G. top-layer dew and sublimation
    if snl == 0:
        mark("snl_0")
        liq[0] = liq[0] + (1.0 - frac_h2osfc) * c["qflx_dew_grnd"] * dt
        ice[0] = ice[0] + (1.0 - frac_h2osfc) * c["qflx_dew_snow"] * dt
        if c["qflx_sub_snow"] * dt > ice[0]:
            ice[0] = 0.0
        else:
            ice[0] = ice[0] - (1.0 - frac_h2osfc) * c["qflx_sub_snow"] * dt
    else:
        mark("snl_pos")

    # H. stores
    volnew = [_div(liq[j], dz[j] * DENH2O) + _div(ice[j], dz[j] * DENICE) for j in range(N)]
    o = {"liq": liq, "ice0": ice[0], "vol": volnew, "h2osfc": h2osfc, "zwt": _canon(zwt), "wa": _canon(wa),
         "qflx_surf": _canon(qflx_surf), "qflx_infl": _canon(infl), "qflx_h2osfc_surf": _canon(qs), "qflx_drain": _canon(qflx_drain),
         "qflx_rsub_sat": _canon(rsub_sat), "qcharge": _canon(qcharge), "fsat": _canon(fsat)}
    if frost:
        o["frost_table"], o["zwt_perched"], o["qflx_drain_perched"] = _canon(ft), _canon(zwp), _canon(qp)
    if rof is not None:
        o["h2orof"], o["frac_h2orof"], o["qflx_h2orof_drain"] = _canon(hr), _canon(fr), _canon(d)
    return o


FPI_H2OROF, FPI_FRAC, FPI_QFLX_DRAIN = range(3)  # ELMK_FPI_*: the floodplain infiltration's column rows
FPI_NROWS = 3


def step(fields, rows, dt, hit=None, stored=None, frost=None, probes=None, rof=None, lat=None):
    """One elmk_soil_hydrology on the host.

    fields: a dict of the state fields READS and h2osoi_vol as S[name] downloads them ([n] or [n, nlev], any float dtype: widened to
    fp64 as stored); rows: float64 [NROWS, n], the rows of the feature (ZWT .. FSAT).  Returns (out, rows_out): out holds the fields
    WRITES in the dtype and shape of the inputs (fp64 results rounded once to the stored type), rows_out the rows after the step
    (parameters unchanged, diagnostics overwritten).  Nothing is changed in place.  hit: see column().  stored: the element type the
    state is stored in where the inputs do not show it - np.float32 for downloads of the fp32-state build, which come widened to fp64:
    the results are rounded to it before they take the inputs' dtype.  frost: float64 [FROST_NROWS, n], the rows of the frost-table
    extension (Q_PERCH_MAX .. QFLX_DRAIN_PERCHED); with it the step takes the F' form, reads t_soisno as well and returns
    (out, rows_out, frost_out), frost_out the extension's rows after the step.  probes: a list that receives column()'s probe of every
    column in turn.  rof=(cellof, wf, flood_frac, area): the floodplain infiltration's form (include/elmk.h "floodplain infiltration",
    F1 - F3): cellof int [n], the cell of every column or -1; wf, flood_frac, area float64 [ncells], the routing's rows as its last call
    left them.  The result grows by fpi_out, float64 [FPI_NROWS, n]: H2OROF, FRAC, QFLX_H2OROF_DRAIN.
    lat=(down, dist, width, area, elev, k_aniso): the hillslope lateral flow's form (include/elmk.h "hillslope lateral flow"): L1 and L2
    from the inputs (hillslope_head, hillslope_flow), then every column with L3.  The result grows by hs_out, float64 [HS_NROWS, n].  It
    excludes frost and rof, as the device does."""
    dt = float(dt)
    if lat is not None:
        assert frost is None and rof is None
        l_down = np.asarray(lat[0]).reshape(-1)
        hs_out = np.zeros((HS_NROWS, l_down.size))
        hs_out[HS_HEAD], hs_out[HS_TRANS] = hillslope_head(fields, rows, l_down, lat[4], lat[5])
        hs_out[HS_QLAT_OUT:] = hillslope_flow(hs_out[HS_HEAD], hs_out[HS_TRANS], l_down, lat[1], lat[2], lat[3], hit=hit)
    if rof is not None:
        r_cell = np.asarray(rof[0]).reshape(-1)
        r_wf, r_ff, r_ar = (np.asarray(x, dtype=np.float64).reshape(-1) for x in rof[1:])
    f = {k: np.asarray(fields[k]) for k in READS + ("h2osoi_vol",) + (("t_soisno",) if frost is not None else ())}
    n = f["h2osfc"].shape[0]
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.shape == (NROWS, n)
    w = {k: (v.astype(np.float64) if v.dtype.kind == "f" else v) for k, v in f.items()}
    out = {k: np.array(f[k]) for k in WRITES}
    res = {k: np.array(w[k], dtype=np.float64) for k in WRITES}
    rows_out = rows.copy()
    if frost is not None:
        frost = np.asarray(frost, dtype=np.float64)
        assert frost.shape == (FROST_NROWS, n)
        frost_out = frost.copy()
    if rof is not None:
        assert r_cell.shape == (n,)
        fpi_out = np.zeros((FPI_NROWS, n))
    s0, s1 = NLEVSNO, NLEVSNO + N
    for i in range(n):
        c = {"liq": w["h2osoi_liq"][i, s0:s1].tolist(), "ice": w["h2osoi_ice"][i, s0:s1].tolist(), "dz": w["dz"][i, s0:s1].tolist(),
             "z": w["zsoi"][i, s0:s1].tolist(), "zi": w["zisoi"][i, s0:s1 + 1].tolist(), "watsat": w["watsat"][i, :N].tolist(),
             "sucsat": w["sucsat"][i, :N].tolist(), "bsw": w["bsw"][i, :N].tolist(), "rootsoi": w["qflx_rootsoi"][i, :N].tolist(),
             "hksat": rows[HKSAT:HKSAT + N, i].tolist(), "snl": int(w["snl"][i]), "fsno": float(w["frac_sno_eff"][i])}
        for k in ("h2osfc", "frac_h2osfc", "qflx_top_soil", "qflx_evap_grnd", "qflx_ev_soil", "qflx_ev_h2osfc", "qflx_dew_grnd",
                  "qflx_dew_snow", "qflx_sub_snow"):
            c[k] = float(w[k][i])
        c["zwt"], c["wa"] = float(rows[ZWT, i]), float(rows[WA, i])
        c["wtfact"], c["h2osfc_thresh"] = float(rows[WTFACT, i]), float(rows[H2OSFC_THRESH, i])
        c["k_wet"], c["rsub_top_max"] = float(rows[K_WET, i]), float(rows[RSUB_TOP_MAX, i])
        if frost is not None:
            c["t"], c["q_perch_max"] = w["t_soisno"][i, s0:s1].tolist(), float(frost[Q_PERCH_MAX, i])
        if rof is not None:
            g = int(r_cell[i])
            c["rof"] = (True, float(r_wf[g]), float(r_ff[g]), float(r_ar[g])) if g >= 0 else (False, 0.0, 0.0, 0.0)
        if lat is not None and int(l_down[i]) != -2:
            c["lat"] = float(hs_out[HS_QLAT_NET, i])
        elif lat is not None and hit is not None:
            hit.add("lat_off_hillslope")
        if probes is None:
            o = column(c, dt, hit)
        else:
            probes.append({})
            o = column(c, dt, hit, probes[-1])
        if frost is not None:
            frost_out[FROST_TABLE, i], frost_out[ZWT_PERCHED, i] = o["frost_table"], o["zwt_perched"]
            frost_out[QFLX_DRAIN_PERCHED, i] = o["qflx_drain_perched"]
        if rof is not None:
            fpi_out[:, i] = o["h2orof"], o["frac_h2orof"], o["qflx_h2orof_drain"]
        res["h2osoi_liq"][i, s0:s1] = o["liq"]
        res["h2osoi_ice"][i, s0] = o["ice0"]
        res["h2osoi_vol"][i, :N] = o["vol"]
        res["h2osfc"][i] = o["h2osfc"]
        rows_out[ZWT, i], rows_out[WA, i] = o["zwt"], o["wa"]
        for d, name in enumerate(DIAGNOSTICS):
            rows_out[QFLX_SURF + d, i] = o[name]
    with np.errstate(all="ignore"):
        # untouched levels keep their stored bits; the written ones are rounded once to the stored type
        def rnd(a, like):
            return (a if stored is None else a.astype(stored)).astype(like.dtype)

        out["h2osoi_liq"][:, s0:s1] = rnd(res["h2osoi_liq"][:, s0:s1], out["h2osoi_liq"])
        out["h2osoi_ice"][:, s0] = rnd(res["h2osoi_ice"][:, s0], out["h2osoi_ice"])
        out["h2osoi_vol"][:, :N] = rnd(res["h2osoi_vol"][:, :N], out["h2osoi_vol"])
        out["h2osfc"][:] = rnd(res["h2osfc"], out["h2osfc"])
    ret = (out, rows_out) if frost is None else (out, rows_out, frost_out)
    if lat is not None:
        return ret + (hs_out,)
    return ret if rof is None else ret + (fpi_out,)


# ---- hillslope lateral flow (include/elmk.h "hillslope lateral flow"; k_hillslope.hip, elmk_maps.h: hillslope_check) --------------
HS_HEAD, HS_TRANS, HS_QLAT_OUT, HS_QLAT_IN, HS_QLAT_NET, HS_QSTREAM = range(6)  # ELMK_HS_*
HS_NROWS = 6
HS_MAXUP = 8


def hillslope_check(down, dist, width, area, elev, k_aniso):
    """elmk_maps.h: hillslope_check on the host, the same checks in the same order with the same texts: returns (text, col) - the
    refusal and the first offending column, -1 where the text is about no column - or (None, -1) for an accepted set.  The entry point's
    message is "elmk_hillslope_enable: <text> at column <col>"."""
    if any(v is None for v in (down, dist, width, area, elev)):
        return "null argument", -1
    down = np.asarray(down).reshape(-1)
    n = down.size
    if n < 1 or n > 2 ** 31 - 1:
        return "ncols outside 1 .. 2^31-1", -1
    d = down.astype(np.int64)
    rows = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (dist, width, area, elev)]

    def first(mask):
        idx = np.nonzero(mask)[0]
        return int(idx[0]) if idx.size else -1

    c = first((d < -2) | (d >= n))
    if c >= 0:
        return "down outside {-2, -1} and [0, ncols)", c
    c = first(d == np.arange(n))
    if c >= 0:
        return "down equals its own index", c
    c = first((d >= 0) & (d[np.maximum(d, 0)] == -2))
    if c >= 0:
        return "down names a column on no hillslope", c
    deg = [0] * n
    for c in range(n):
        if d[c] >= 0:
            if deg[d[c]] == HS_MAXUP:
                return "more than 8 uphill columns drain into one column", c
            deg[d[c]] += 1
    mark = [0] * n
    dl = d.tolist()
    for c in range(n):
        if mark[c]:
            continue
        j = c
        while j >= 0 and mark[j] == 0:
            mark[j] = 1
            j = dl[j]
        if j >= 0 and mark[j] == 1:
            return "the hillslope has a cycle", c
        j = c
        while j >= 0 and mark[j] == 1:
            mark[j] = 2
            j = dl[j]
    on = d != -2
    with np.errstate(invalid="ignore"):
        for name, row in zip(("dist", "width", "area"), rows):
            c = first(on & ~(np.isfinite(row) & (row > 0.0)))
            if c >= 0:
                return name + " not finite and > 0", c
        c = first(on & ~np.isfinite(rows[3]))
    if c >= 0:
        return "elev not finite", c
    k = float(k_aniso)
    if not (math.isfinite(k) and k > 0.0):
        return "k_aniso not finite and > 0", -1
    return None, -1


def hillslope_map(down):
    """The uphill map of an accepted set as the device reads it: int32 [npad, n], npad = 1, 2, 4 or 8 rows; row p holds, for column c,
    the p-th column u with down[u] == c in ascending u, else -1."""
    d = np.asarray(down).reshape(-1).astype(np.int64)
    n = d.size
    slots = [[] for _ in range(n)]
    for u in range(n):
        if d[u] >= 0:
            slots[d[u]].append(u)
    most = max((len(v) for v in slots), default=0)
    npad = 1 if most <= 1 else 2 if most <= 2 else 4 if most <= 4 else 8
    up = np.full((npad, n), -1, dtype=np.int32)
    for c, v in enumerate(slots):
        up[:len(v), c] = v
    return up


def hillslope_head(fields, rows, down, elev, k_aniso):
    """L1 on the host: (HEAD [n], TRANS [n]) from the state fields (h2osoi_ice, dz, zisoi, watsat as S[name] downloads them) and the
    hydrology's rows [NROWS, n] at the start of the stage."""
    rows = np.asarray(rows, dtype=np.float64)
    down = np.asarray(down).reshape(-1)
    n = down.size
    elev = np.broadcast_to(np.asarray(elev, dtype=np.float64), (n,))
    k_aniso = float(k_aniso)
    w = {k: np.asarray(fields[k]).astype(np.float64) for k in ("h2osoi_ice", "dz", "zisoi", "watsat")}
    head, trans = np.zeros(n), np.zeros(n)
    s0, s1 = NLEVSNO, NLEVSNO + N
    for c in range(n):
        if int(down[c]) == -2:
            continue
        zwt = float(rows[ZWT, c])
        ice, dz = w["h2osoi_ice"][c, s0:s1].tolist(), w["dz"][c, s0:s1].tolist()
        zi, watsat = w["zisoi"][c, s0:s1 + 1].tolist(), w["watsat"][c, :N].tolist()
        hksat = rows[HKSAT:HKSAT + N, c].tolist()
        jwt = _jwt(zwt, zi)
        t = 0.0
        if jwt < N:
            si, sd = 0.0, 0.0
            for j in range(_max(jwt - 1, 0), N):
                vol_ice = _min(watsat[j], _div(ice[j], dz[j] * DENICE))
                icefrac = _min(1.0, _div(vol_ice, watsat[j]))
                dzmm = dz[j] * 1.0e3
                si = si + icefrac * dzmm
                sd = sd + dzmm
            imp = _pow(10.0, -E_ICE * _div(si, sd))
            for j in range(jwt, N):
                t = t + hksat[j] * (zi[j + 1] - zwt if j == jwt else dz[j])
            t = imp * t * 1.0e-3 * k_aniso
        head[c] = _canon(float(elev[c]) - zwt)
        trans[c] = _canon(t)
    return head, trans


def _hs_vol(d, hu, tu, hd, td, dist, width, hit=None):
    """L2: the flux of the edge out of a column, m3/s; d its down (-1: the stream), hd and td HEAD and TRANS of d."""
    if d == -1:
        g = _max(_div(hu, dist), 0.0)
        if hit is not None:
            hit.add("lat_stream_clamp" if not hu > 0.0 else "lat_stream")
    else:
        g = _div(hu - hd, dist)
    if hit is not None:
        if g < -2.0:
            hit.add("lat_clamp_lo")
        if g > 2.0:
            hit.add("lat_clamp_hi")
        if d != -1 and g > 0.0:
            hit.add("lat_g_pos")
        if d != -1 and g < 0.0:
            hit.add("lat_g_neg")
    g = _min(_max(g, -2.0), 2.0)
    t = td if (d != -1 and g < 0.0) else tu
    return t * width * g


def hillslope_flow(head, trans, down, dist, width, area, up=None, hit=None):
    """L2 on the host: float64 [4, n], QLAT_OUT, QLAT_IN, QLAT_NET, QSTREAM.  up: hillslope_map(down), or None to build it."""
    head, trans = (np.asarray(v, dtype=np.float64).tolist() for v in (head, trans))
    down = np.asarray(down).reshape(-1).astype(np.int64).tolist()
    n = len(down)
    dist, width, area = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)).tolist() for v in (dist, width, area))
    up = hillslope_map(down) if up is None else np.asarray(up)
    out = np.zeros((4, n))
    for c in range(n):
        d = down[c]
        if d == -2:
            continue
        hd, td = (head[d], trans[d]) if d >= 0 else (0.0, 0.0)
        vol = _hs_vol(d, head[c], trans[c], hd, td, dist[c], width[c], hit)
        qo = _div(1.0e3 * vol, area[c])
        qi = 0.0
        for p in range(up.shape[0]):
            u = int(up[p, c])
            if u >= 0:
                qi = qi + _div(1.0e3 * _hs_vol(c, head[u], trans[u], head[c], trans[c], dist[u], width[u]), area[c])
        out[:, c] = _canon(qo), _canon(qi), _canon(qo - qi), _canon(vol if d == -1 else 0.0)
    return out


def hillslope_budget(qstream):
    """elmk_hillslope_budget on the host: float64 [1], the sum of QSTREAM in the device reduction's order
    (diagnostics.reduce_min_max_sum)."""
    from .diagnostics import reduce_min_max_sum

    q = np.asarray(qstream, dtype=np.float64).reshape(-1)
    return np.array([reduce_min_max_sum(q)[2] if q.size else 0.0])


# ---- parameters -------------------------------------------------------------------------------------------------------------------
def hksat_from_texture(pct_sand, pct_clay, organic, zsoi, organic_max=130.0):
    """ELM's saturated hydraulic conductivity (mm/s): the Cosby pedotransfer for the mineral part mixed with the organic part above
    the percolation threshold (iniTimeConst).  pct_sand, pct_clay, organic (kg/m3), zsoi (m): [n, 10] or broadcastable; returns
    float64 [10, n], the layout of soil_hydrology_set_params."""
    sand, clay, om, z = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (pct_sand, pct_clay, organic, zsoi)))
    shape = sand.shape
    out = np.empty(sand.size)
    pcalpha, pcbeta = 0.5, 0.139
    for i, (s, _c, o, zz) in enumerate(zip(sand.reshape(-1), clay.reshape(-1), om.reshape(-1), z.reshape(-1))):
        s, o, zz = float(s), float(o), float(zz)
        om_frac = _min(o / organic_max, 1.0)
        xksat = 0.0070556 * _pow(10.0, -0.884 + 0.0153 * s)
        om_hksat = _max(0.28 - 0.2799 * zz / 0.5, 0.0001)
        if om_frac > pcalpha:
            perc_norm = _pow(1.0 - pcalpha, -pcbeta)
            perc_frac = perc_norm * _pow(om_frac - pcalpha, pcbeta)
        else:
            perc_frac = 0.0
        uncon_frac = (1.0 - om_frac) + (1.0 - perc_frac) * om_frac
        if om_frac < 1.0:
            uncon_hksat = uncon_frac / ((1.0 - om_frac) / xksat + ((1.0 - perc_frac) * om_frac) / om_hksat)
        else:
            uncon_hksat = 0.0
        out[i] = uncon_frac * uncon_hksat + (perc_frac * om_frac) * om_hksat
    out = out.reshape(shape)
    return np.ascontiguousarray(out.T if out.ndim == 2 else out.reshape(N, -1))


def h2osfc_thresh(micro_sigma):
    """ELM's surface-water threshold (mm) from the microtopography's standard deviation (m): four Newton iterations for the depth d
    at which the inundated fraction reaches pc, then the mean water depth over that fraction."""
    sig = np.asarray(micro_sigma, dtype=np.float64)
    out = np.empty(sig.size)
    for i, s in enumerate(sig.reshape(-1)):
        s = float(s)
        if s > 1.0e-6:
            d = 0.0
            for _ in range(4):
                fd = 0.5 * (1.0 + math.erf(d / (s * math.sqrt(2.0)))) - PC
                dfdd = math.exp(-d * d / (2.0 * s * s)) / (s * math.sqrt(2.0 * math.pi))
                d = d - fd / dfdd
            out[i] = 0.5 * d * (1.0 + math.erf(d / (s * math.sqrt(2.0)))) + s / math.sqrt(2.0 * math.pi) * math.exp(-d * d / (2.0 * s * s))
            out[i] = 1.0e3 * out[i]
        else:
            out[i] = 0.0
    return out.reshape(sig.shape)


def k_wet(topo_slope_deg):
    """sin of the slope (given in degrees, as ELM's surface data holds it)."""
    a = np.asarray(topo_slope_deg, dtype=np.float64)
    return np.array([math.sin(float(v) * (math.pi / 180.0)) for v in a.reshape(-1)]).reshape(a.shape)


def rsub_top_max(topo_slope_deg):
    """The maximum baseflow rate (mm/s): 10 sin(slope)."""
    return 10.0 * k_wet(topo_slope_deg)


def q_perch_max(topo_slope_deg):
    """The perched drainage's rate parameter (1/s): 1e-5 sin(slope).  Evaluated on the host, so that the device needs no sin."""
    return 1.0e-5 * k_wet(topo_slope_deg)


def water_balance_error(begwb, endwb, wa_beg, wa_end, forc_rain, forc_snow, qflx_evap_tot, qflx_snwcp_ice, qflx_surf, qflx_h2osfc_surf,
                        qflx_drain, dt, qflx_drain_perched=None, qflx_irrig=None):
    """The reference's column_water_balance_error with the aquifer in both water masses and
    hydrology_source_sink = qflx_surf + qflx_h2osfc_surf + qflx_drain in place of its hardwired 0:
    errh2o = (endwb + wa_end) - (begwb + wa_beg) - (forc_rain + forc_snow - source_sink - qflx_evap_tot - qflx_snwcp_ice) * dt.
    qflx_drain_perched: the frost-table extension's lateral drainage, one more term of the source/sink.  qflx_irrig: the irrigation's
    applied rate, one more term of the input: (forc_rain + forc_snow) + qflx_irrig (ELM's BalanceCheck)."""
    a = [np.asarray(v, dtype=np.float64) for v in (begwb, endwb, wa_beg, wa_end, forc_rain, forc_snow, qflx_evap_tot, qflx_snwcp_ice,
                                                   qflx_surf, qflx_h2osfc_surf, qflx_drain)]
    begwb, endwb, wa_beg, wa_end, rain, snow, evap, snwcp, surf, h2osfc_surf, drain = a
    source_sink = surf + h2osfc_surf + drain
    if qflx_drain_perched is not None:
        source_sink = source_sink + np.asarray(qflx_drain_perched, dtype=np.float64)
    if qflx_irrig is not None:
        return (endwb + wa_end) - (begwb + wa_beg) - (((rain + snow) + np.asarray(qflx_irrig, dtype=np.float64)) - source_sink - evap - snwcp) * float(dt)
    return (endwb + wa_end) - (begwb + wa_beg) - (rain + snow - source_sink - evap - snwcp) * float(dt)


# ---- water balance (include/elmk.h "water balance"; k_water_balance.hip) ----------------------------------------------------------
# the rows of the feature (ELMK_WB_*)
WB_BEGWB, WB_ERRH2O, WB_QRUNOFF, WB_ENDWB, WB_SOILWATER_10CM, WB_TOTSOILLIQ, WB_TOTSOILICE = range(7)
WB_NROWS = 7
NLEVTOT = 20
# the state fields W1 - W6 read
WB_READS = ("h2ocan", "h2osno", "h2osfc", "h2osoi_ice", "h2osoi_liq", "zisoi", "dz", "qflx_snwcp_liq", "forc_rain", "forc_snow",
            "qflx_evap_tot", "qflx_snwcp_ice")


def _wb_canon(a):
    a = np.array(a, dtype=np.float64)
    a[a != a] = _NAN
    return a


def _wide(fields, names):
    return {k: np.asarray(fields[k]).astype(np.float64) for k in names}


def water_balance_begin(fields, rows, wb=None):
    """W0 on the host: BEGWB = dtbegin_column_h2o + WA.  fields: S[name] downloads (widened to fp64 as stored); rows: float64
    [NROWS, n], the hydrology's rows; wb: float64 [WB_NROWS, n] or None for zeros.  Returns the rows of the feature after the call."""
    rows = np.asarray(rows, dtype=np.float64)
    n = rows.shape[1]
    out = np.zeros((WB_NROWS, n)) if wb is None else np.array(wb, dtype=np.float64)
    with np.errstate(all="ignore"):
        out[WB_BEGWB] = _wb_canon(np.asarray(fields["dtbegin_column_h2o"]).astype(np.float64) + rows[WA])
    return out


def water_balance_end(fields, rows, wb, dt, frost=None, snwcp_liq_term=True, qflx_irrig=None, qflx_h2orof_drain=None):
    """W1 - W6 on the host, one numpy operation per IEEE operation in the header's order.  fields: the state fields WB_READS as S[name]
    downloads them; rows: the hydrology's rows after the step's soil_hydrology; wb: the rows of the feature, BEGWB from
    water_balance_begin; frost: the frost-table extension's rows [FROST_NROWS, n] where it is enabled.  Returns the rows after the
    stage (BEGWB unchanged).  snwcp_liq_term=False leaves W3's last term out (a measurement, not the stage).  qflx_irrig: the
    irrigation's QFLX_IRRIG row [n] where that feature is enabled: W4 takes (forc_rain + forc_snow) + qflx_irrig as the input.
    qflx_h2orof_drain: the floodplain infiltration's QFLX_H2OROF_DRAIN row [n] where that extension is on: the input's last term (F4)."""
    dt = float(dt)
    rows, wb = np.asarray(rows, dtype=np.float64), np.array(wb, dtype=np.float64)
    w = _wide(fields, WB_READS)
    ice, liq = w["h2osoi_ice"], w["h2osoi_liq"]
    with np.errstate(all="ignore"):
        water = w["h2ocan"] + w["h2osno"] + w["h2osfc"]  # W1
        for i in range(NLEVTOT):
            water = water + (ice[:, i] + liq[:, i])
        endwb = water + rows[WA]  # W2
        q = rows[QFLX_SURF] + rows[QFLX_H2OSFC_SURF] + rows[QFLX_DRAIN]  # W3
        if frost is not None:
            q = q + np.asarray(frost, dtype=np.float64)[QFLX_DRAIN_PERCHED]
        qrunoff = q + w["qflx_snwcp_liq"] if snwcp_liq_term else q
        if qflx_h2orof_drain is not None:
            inp = w["forc_rain"] + w["forc_snow"]
            if qflx_irrig is not None:
                inp = inp + np.asarray(qflx_irrig, dtype=np.float64)
            inp = inp + np.asarray(qflx_h2orof_drain, dtype=np.float64)
            err = endwb - wb[WB_BEGWB] - (inp - qrunoff - w["qflx_evap_tot"] - w["qflx_snwcp_ice"]) * dt
        elif qflx_irrig is None:
            err = endwb - wb[WB_BEGWB] - (w["forc_rain"] + w["forc_snow"] - qrunoff - w["qflx_evap_tot"] - w["qflx_snwcp_ice"]) * dt  # W4
        else:
            qi = np.asarray(qflx_irrig, dtype=np.float64)
            err = endwb - wb[WB_BEGWB] - (((w["forc_rain"] + w["forc_snow"]) + qi) - qrunoff - w["qflx_evap_tot"] - w["qflx_snwcp_ice"]) * dt
        n = water.shape[0]
        totliq, totice, s = np.zeros(n), np.zeros(n), np.zeros(n)
        zi = w["zisoi"][:, NLEVSNO:NLEVSNO + N + 1]  # zi[:, 0] = the surface, zi[:, j + 1] = the bottom of layer j
        for j in range(N):  # W5, W6
            lj, ij = liq[:, NLEVSNO + j], ice[:, NLEVSNO + j]
            totliq = totliq + lj
            totice = totice + ij
            whole = zi[:, j + 1] <= 0.1
            part = ~whole & (zi[:, j] < 0.1)
            s = np.where(whole, s + (lj + ij), np.where(part, s + (lj + ij) * ((0.1 - zi[:, j]) / w["dz"][:, NLEVSNO + j]), s))
    wb[WB_ERRH2O], wb[WB_QRUNOFF], wb[WB_ENDWB] = _wb_canon(err), _wb_canon(qrunoff), _wb_canon(endwb)
    wb[WB_SOILWATER_10CM], wb[WB_TOTSOILLIQ], wb[WB_TOTSOILICE] = _wb_canon(s), _wb_canon(totliq), _wb_canon(totice)
    return wb


def water_balance_reduce(wb, tol):
    """W7 and W8 on the host: ((min, max, sum) [3, 3] of ERRH2O, QRUNOFF, ENDWB in the device reduction's order
    (diagnostics.reduce_min_max_sum), nbad, first_bad_col).  No columns: (+inf, -inf, +0.0), 0, -1."""
    from .diagnostics import reduce_min_max_sum

    wb = np.asarray(wb, dtype=np.float64)
    if wb.shape[1] == 0:
        return np.tile(np.array([np.inf, -np.inf, 0.0]), (3, 1)), 0, -1
    mms = np.stack([reduce_min_max_sum(wb[k]) for k in (WB_ERRH2O, WB_QRUNOFF, WB_ENDWB)])
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(wb[WB_ERRH2O]) <= float(tol))
    idx = np.nonzero(bad)[0]
    return mms, int(idx.size), int(idx[0]) if idx.size else -1
