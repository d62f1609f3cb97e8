"""Physical checks of the soil hydrology's host truth (elmkernels_amd/hydrology.py: column).  The device is held to the host bit for bit
and the host's water budget telescopes for any consistent set of fluxes, so neither says that the fluxes are the right ones.  Here the
references are written from the physics in mpmath at 40 digits - the Clapp-Hornberger retention curve, Darcy's law relative to the
hydrostatic profile, the closed forms of the runoff and the drainage - and not from column()'s statements:

a. a column in hydrostatic equilibrium with its water table (layer means of the equilibrium profile by quadrature) stays put;
b. the interface fluxes q and the right-hand sides r of an unsaturated column are Darcy's, and the change of the soil water over a
   vanishing step tends to r;
c. dq1 and dq2 are the derivatives of that flux, and the Thomas solve leaves a residual of rounding size;
d. fsat, the baseflow, the water it removes and the fall of the water table are their closed forms.

Every tolerance is derived from the rounding of the operations it covers (U = 2^-53, the condition of pow: a relative error e of the
base becomes |exponent| * e) and the measured value is recorded beside it."""
import math

import mpmath as mp
import numpy as np
import pytest

from elmkernels_amd import hydrology as hy
from tests.hydrology_cases import DT, column, edge_columns, edge_finite

mp.mp.dps = 40
N = hy.N
U = 2.0 ** -53
ZI = column()["zi"]
ZIMM = [mp.mpf(v) * 1000 for v in ZI]
ZMM = [mp.mpf(v) * 1000 for v in column()["z"]]

UNIFORM = dict(bsw=[5.0] * N, sucsat=[200.0] * N, watsat=[0.45] * N)
LAYERED = dict(bsw=[2.8, 9.5, 4.2, 6.0, 3.3, 8.1, 5.0, 7.4, 3.9, 6.6], sucsat=[12.0, 180.0, 35.0, 90.0, 207.0, 20.0, 150.0, 60.0, 110.0, 45.0],
               watsat=[0.9, 0.43, 0.7, 0.5, 0.62, 0.45, 0.8, 0.55, 0.47, 0.66])
OTHER = dict(bsw=[9.5] * N, sucsat=[12.0] * N, watsat=[0.6] * N)


# ---- the reference: the hydrostatic profile and Darcy's law, in 40 digits -------------------------------------------------------------
def theta_eq(z, zwt, par, j):
    """The equilibrium water content at depth z (mm) of layer j over a water table at zwt (mm)."""
    w, s, b = mp.mpf(par["watsat"][j]), mp.mpf(par["sucsat"][j]), mp.mpf(par["bsw"][j])
    return w if z >= zwt else w * ((s + zwt - z) / s) ** (-1 / b)


def layer_mean(a, b_, zwt, par, j):
    """The mean of theta_eq over [a, b_] by quadrature (the profile has a kink at the water table: split there)."""
    pts = [a, b_] if not a < zwt < b_ else [a, zwt, b_]
    return mp.quad(lambda z: theta_eq(z, zwt, par, j), pts) / (b_ - a)


def psi(theta, par, j):
    """The matric potential (mm) of water content theta in layer j."""
    return -mp.mpf(par["sucsat"][j]) * (theta / mp.mpf(par["watsat"][j])) ** (-mp.mpf(par["bsw"][j]))


def equilibrium_potentials(zwt_m, par):
    """psi of the layer means of the hydrostatic profile, and for a table below the column that of the aquifer node (the bottom
    layer's soil between the column's bottom and the table)."""
    zwt = mp.mpf(zwt_m) * 1000
    pe = [psi(layer_mean(ZIMM[j], ZIMM[j + 1], zwt, par, j), par, j) for j in range(N)]
    if zwt > ZIMM[N]:
        pe.append(psi(layer_mean(ZIMM[N], zwt, zwt, par, N - 1), par, N - 1))
    return pe


def darcy(theta, zwt_m, par, hksat, pe=None):
    """-> (q, r): the flux (mm/s, positive downwards) through the interface below node i = 0 .. N - 1 and the right-hand side of node
    j = 0 .. N (N: the aquifer node) for an ice-free profile theta without sources.  Interface conductivity from the mean saturation of
    the two nodes, psi = -sucsat s^-bsw, the gradient relative to the equilibrium potentials.  With the table inside the column the
    bottom is sealed."""
    zwt = mp.mpf(zwt_m) * 1000
    pe = equilibrium_potentials(zwt_m, par) if pe is None else pe
    below = zwt > ZIMM[N]
    p = [psi(theta[j], par, j) for j in range(N)]
    q = []
    for i in range(N):
        ip = min(i + 1, N - 1)
        s = (theta[i] + theta[ip]) / (mp.mpf(par["watsat"][i]) + mp.mpf(par["watsat"][ip]))
        k = mp.mpf(hksat[i]) * s ** (2 * mp.mpf(par["bsw"][i]) + 3)
        if i < N - 1:
            q.append(-k * ((p[i + 1] - p[i]) - (pe[i + 1] - pe[i])) / (ZMM[i + 1] - ZMM[i]))
        elif below:  # the aquifer node holds the bottom layer's water: its potential is the bottom layer's
            zn = (zwt + ZMM[N - 1]) / 2
            q.append(-k * ((p[N - 1] - p[N - 1]) - (pe[N] - pe[N - 1])) / (zn - ZMM[N - 1]))
        else:
            q.append(mp.mpf(0))
    r = [-q[0]] + [q[j - 1] - q[j] for j in range(1, N)] + [q[N - 1] if below else mp.mpf(0)]
    return q, r


def build(theta, zwt_m, par, hksat, **kw):
    """The column of hydrology_cases.column with these parameters and liq = theta * dz in mm (rounded to fp64 once each)."""
    c = column(zwt=float(zwt_m), hksat=0.0, **kw)
    c.update(bsw=list(par["bsw"]), sucsat=list(par["sucsat"]), watsat=list(par["watsat"]), hksat=list(hksat))
    c["liq"] = [float(theta[j]) * (c["dz"][j] * 1.0e3) for j in range(N)]
    return c


# ---- the rounding model ---------------------------------------------------------------------------------------------------------------
def potential_errors(c, zwt_m, par, pe):
    """Bounds (mm) on the rounding error of smp[j] and of zq[j] as column() evaluates them, in units of 1: multiply by U.

    smp[j] = -sucsat * s^-bsw with s from liq through five roundings (the reference rounded to fp64, liq = theta * dzmm, dz * 1000,
    the division by it, the division by watsat): s carries 5 U, pow turns that into 5 bsw U and adds its own (under 1 ulp = 2 U), the
    product one more: (5 bsw + 3) |smp|.

    zq[j] = -sucsat * (ve / watsat)^-bsw with ve from the closed form of the layer mean, a multiple of the difference of two powers
    t = ((sucsat + zwt - z) / sucsat)^b1 taken at the layer's two interfaces (at the table, 1).  Each base carries 5 U (two products
    by 1000, a sum, a difference, a division), the exponent b1 = 1 - 1 / bsw carries 2 U, which pow turns into 2 b1 ln(base) U: with
    pow's own 2 U each power carries KT = 5 b1 + 2 b1 ln(base) + 2.  Their difference cancels: relative to it the error is KT times
    A = (t0 + t1) / |t0 - t1|, which reaches several hundred where a thin layer lies far above the table.  The factor in front adds 6
    roundings and in the table's own layer the weighted mean 4 more; the division by watsat, pow and the product as for smp:
    (bsw (KT A + 11) + 3) |zq|.  In a layer below the table ve = watsat and zq = -sucsat exactly."""
    zwt = mp.mpf(zwt_m) * 1000
    e_smp, e_zq = [], []
    for j in range(N + (1 if len(pe) > N else 0)):
        k = min(j, N - 1)
        b, s = par["bsw"][k], mp.mpf(par["sucsat"][k])
        top, bot = (ZIMM[j], ZIMM[j + 1]) if j < N else (ZIMM[N], zwt)
        if j < N:
            e_smp.append((5 * b + 3) * abs(float(psi(mp.mpf(c["liq"][j]) / (mp.mpf(c["dz"][j]) * 1000), par, j))))
        if zwt <= top:
            e_zq.append(0.0)
            continue
        b1 = 1 - 1 / mp.mpf(b)
        t0 = ((s + zwt - top) / s) ** b1
        t1 = ((s + zwt - min(bot, zwt)) / s) ** b1
        kt = 5 * b1 + 2 * b1 * mp.log((s + zwt - top) / s) + 2
        amp = (t0 + t1) / abs(t0 - t1)
        e_zq.append(float((b * (kt * amp + 11) + 3) * abs(pe[j])))
    return e_smp, e_zq


def flux_errors(c, zwt_m, par, hksat, theta, pe, q):
    """Bounds (mm/s, in units of U) on the rounding error of q[i]: the conductivity k = hksat s^(2 bsw + 3) carries
    ((2 bsw + 3) 4 + 5) of its value (s from two liq of 4 roundings each, a sum and a division; pow, two products), which goes with
    |q|; the head difference carries the errors of its four potentials plus its three subtractions (3 U of the largest potential),
    which goes with k / dz; the division and the product two more."""
    e_smp, e_zq = potential_errors(c, zwt_m, par, pe)
    out = []
    for i in range(N):
        ip = min(i + 1, N - 1)
        s = (theta[i] + theta[ip]) / (mp.mpf(par["watsat"][i]) + mp.mpf(par["watsat"][ip]))
        k = float(mp.mpf(hksat[i]) * s ** (2 * mp.mpf(par["bsw"][i]) + 3))
        if i < N - 1:
            den = float(ZMM[i + 1] - ZMM[i])
            head = e_smp[i] + e_smp[i + 1] + e_zq[i] + e_zq[i + 1] + 3 * max(abs(float(pe[i])), abs(float(pe[i + 1])), e_smp[i] / 3, e_smp[i + 1] / 3)
        elif len(pe) > N:
            den = float((mp.mpf(zwt_m) * 1000 + ZMM[N - 1]) / 2 - ZMM[N - 1])
            head = 2 * e_smp[i] + e_zq[i] + e_zq[N] + 3 * max(abs(float(pe[N - 1])), abs(float(pe[N])))
        else:
            out.append(0.0)
            continue
        out.append(k / den * head + ((2 * par["bsw"][i] + 3) * 4 + 7) * abs(float(q[i])))
    return out


# ---- a. hydrostatic stationarity -----------------------------------------------------------------------------------------------------
HKSAT = 0.005
# Measured, the restatement against the quadrature reference over the thirty columns below (fp64, glibc pow): the largest |dliq| / liq,
# |qcharge| (mm/s) and |dzwt| (m), and the largest of each relative to its derived bound.  Recorded, not asserted: the bounds are the
# assertion.  The wrong references move a layer by up to 7.9e9 .. 2.1e12 times its bound (per parameter set and reference).
STATIONARY_MEASURED = dict(dliq=1.264e-14, qcharge=6.740e-16, dzwt=6.066e-14, dliq_of_bound=0.016, qcharge_of_bound=0.090, dzwt_of_bound=0.090)


def table_depths():
    """A water table in each of the ten layers, off the middle."""
    return [ZI[j] + 0.37 * (ZI[j + 1] - ZI[j]) for j in range(N)]


def stationary_bounds(c, zwt_m, par):
    """-> (per layer the bound on |dliq| / liq, the bound on |qcharge|, the bound on |dzwt|) for a column in equilibrium.

    At equilibrium the head difference of every interface is zero, so q[i] is its rounding error alone: hk[i] / den[i] times the
    errors of the four potentials (potential_errors).  The solve is (dzmm / dt) u + J u = r with J the flux-difference operator: at
    equilibrium its columns sum to zero, its diagonal is positive and its off-diagonals are negative (dq1 = hk dsmpdw / den > 0,
    dq2 < 0), an M-matrix, so sum |dliq| <= dt sum |r| <= 2 dt sum |q[i]|, and no layer changes by more than that.  F's excess pass
    moves at most the rounding of liq (4 U).  The recharge is ka (smp - zq) / (2000 (zwt - z_above)) of the layer above the table's
    (in layer 0: / (1000 (zwt + 0.001)), with ka <= hksat, and the table moves by qcharge dt / 1000 / sy, sy >= 0.02, plus the
    rounding of its own update."""
    pe = equilibrium_potentials(zwt_m, par)
    theta = [mp.mpf(c["liq"][j]) / (mp.mpf(c["dz"][j]) * 1000) for j in range(N)]
    q0 = [mp.mpf(0)] * N
    eq = flux_errors(c, zwt_m, par, c["hksat"], theta, pe, q0)
    total = 2.0 * DT * sum(eq) * U
    dliq = [total / c["liq"][j] + 4 * U * 2 for j in range(N)]
    jwt = hy._jwt(zwt_m, ZI)
    e_smp, e_zq = potential_errors(c, zwt_m, par, pe)
    up = max(jwt - 1, 0)
    dist = (zwt_m + 1.0e-3) * 1000.0 if jwt == 0 else (zwt_m - c["z"][jwt - 1]) * 2000.0
    qcharge = max(c["hksat"]) * (e_smp[up] + e_zq[up] + abs(float(pe[up]))) * U / dist * (1 + 8 * U)
    dzwt = qcharge * DT / 1000.0 / hy.ROUS_MIN + 4 * U * 2 * zwt_m
    return dliq, qcharge, dzwt


def equilibrium_column(zwt_m, par, how="mean"):
    zwt = mp.mpf(zwt_m) * 1000
    theta = []
    for j in range(N):
        if how == "midpoint":  # wrong: the profile at the node in place of the layer mean
            theta.append(theta_eq(ZMM[j], zwt, par, j))
        elif how == "above" and ZIMM[j] < zwt < ZIMM[j + 1]:  # wrong: the unsaturated branch over the whole of the table's layer
            w, s, b = mp.mpf(par["watsat"][j]), mp.mpf(par["sucsat"][j]), mp.mpf(par["bsw"][j])
            theta.append(mp.quad(lambda z: w * ((s + abs(zwt - z)) / s) ** (-1 / b), [ZIMM[j], zwt, ZIMM[j + 1]]) / (ZIMM[j + 1] - ZIMM[j]))
        else:
            theta.append(layer_mean(ZIMM[j], ZIMM[j + 1], zwt, par, j))
    c = build(theta, zwt_m, par, [HKSAT] * N)
    if how == "total":  # wrong: where there is ice, the equilibrium taken for the total water: a tenth of it frozen
        for j in range(N):
            if ZIMM[j + 1] <= zwt:
                c["ice"][j] = 0.1 * c["liq"][j] * 0.917
                c["liq"][j] = 0.9 * c["liq"][j]
    return c


def departure(c, zwt_m, par):
    """One step -> (the largest |dliq| / liq relative to its bound, |qcharge| and |dzwt| relative to theirs; the same, absolute)."""
    bl, bq, bz = stationary_bounds(c, zwt_m, par)
    o = hy.column(c, DT)
    rel = [abs(o["liq"][j] - c["liq"][j]) / c["liq"][j] for j in range(N)]
    return (max(r / b for r, b in zip(rel, bl)), abs(o["qcharge"]) / bq, abs(o["zwt"] - zwt_m) / bz), (max(rel), abs(o["qcharge"]), abs(o["zwt"] - zwt_m)), max(bl)


@pytest.mark.parametrize("name, par", [("uniform", UNIFORM), ("layered", LAYERED), ("fine-textured", OTHER)])
def test_a_hydrostatic_column_stays_put(name, par):
    """A water table in each of the ten layers; no ice, hksat = 0.005 mm/s everywhere, no forcing, no drainage; liq = the layer mean
    of the equilibrium profile by 40-digit quadrature.  Every layer's water, the recharge and the water table stay inside the derived
    bounds (stationary_bounds); three wrong references - the profile at the node in place of the layer mean, the unsaturated branch
    over the whole of the table's layer, and the equilibrium taken for liquid plus ice where a tenth of the water is frozen - move some
    layer by more than a thousand times its bound.

    The table is kept inside the column: with it below, CLM4.5's aquifer row has a flux at equilibrium (the bottom layer's own
    potential stands in for the aquifer node's, against zq[N]), so there is nothing to assert there."""
    worst = [0.0, 0.0, 0.0]
    worst_abs = [0.0, 0.0, 0.0]
    loosest = 0.0
    for zwt_m in table_depths():
        c = equilibrium_column(zwt_m, par)
        assert not any(c["ice"]) and c["rsub_top_max"] == 0.0 and c["qflx_top_soil"] == 0.0
        ratio, absolute, bound = departure(c, zwt_m, par)
        worst = [max(a, b) for a, b in zip(worst, ratio)]
        worst_abs = [max(a, b) for a, b in zip(worst_abs, absolute)]
        loosest = max(loosest, bound)
        assert max(ratio) <= 1.0, (zwt_m, ratio, absolute)
    print(f"{name}: largest |dliq|/liq {worst_abs[0]:.3e} ({worst[0]:.3f} of its bound; loosest bound {loosest:.3e}), |qcharge| {worst_abs[1]:.3e} mm/s "
          f"({worst[1]:.3f}), |dzwt| {worst_abs[2]:.3e} m ({worst[2]:.3f})")
    for how in ("midpoint", "above", "total"):
        moved = 0.0
        for zwt_m in table_depths()[2::3]:  # (layers 2, 5 and 8: over a table in layer 0 the wrong references have no layer to differ in)
            c = equilibrium_column(zwt_m, par, how)
            ratio, absolute, _ = departure(c, zwt_m, par)
            moved = max(moved, ratio[0])
            assert ratio[0] > 1.0e3, (how, zwt_m, ratio, absolute)
        print(f"{name}: wrong reference '{how}' moves a layer by {moved:.3e} times its bound")


# ---- b. Darcy fluxes; c. their derivatives and the solve -----------------------------------------------------------------------------
def random_columns(count, seed, smin=0.3, smax=0.95):
    """Ice-free unsaturated columns: random saturation profiles, parameters in the ranges of the generator's tier B, the table inside
    the column or below it.  s >= 0.3 keeps every potential above SMPMIN (207 * 0.3^-9.6 = 2e7 mm)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        par = dict(bsw=rng.uniform(2.8, 9.6, N).tolist(), sucsat=rng.uniform(10.0, 207.0, N).tolist(), watsat=rng.uniform(0.43, 0.93, N).tolist())
        hksat = rng.uniform(1.0e-3, 2.0e-2, N).tolist()
        sat = rng.uniform(smin, smax, N)
        theta = [mp.mpf(float(sat[j])) * mp.mpf(par["watsat"][j]) for j in range(N)]
        zwt_m = float(rng.uniform(0.4, 3.6)) if i % 3 else float(rng.uniform(4.0, 9.0))
        out.append((theta, zwt_m, par, hksat))
    return out


@pytest.fixture(scope="module")
def darcy_columns():
    out = []
    for theta, zwt_m, par, hksat in random_columns(18, 11):
        c = build(theta, zwt_m, par, hksat)
        th = [mp.mpf(c["liq"][j]) / (mp.mpf(c["dz"][j]) * 1000) for j in range(N)]  # the water column() is handed, exactly
        pe = equilibrium_potentials(zwt_m, par)
        q, r = darcy(th, zwt_m, par, hksat, pe)
        probe = {}
        hy.column(c, DT, probe=probe)
        out.append((c, th, zwt_m, par, hksat, pe, q, r, probe))
    return out


# Measured on these columns: the largest |q - Darcy| is 0.217 of its bound, the largest |dq - d(flux)/d(theta)| 0.183 of its bound, the
# largest residual of the solve 7.8e-17 (1.5e-16 over the edge tier's finite columns) against 18 * 2^-52 * 11 = 4.4e-14.
FLUX_MEASURED = dict(q_of_bound=0.217, dq_of_bound=0.183, residual=7.824e-17, residual_edge_tier=1.505e-16)


def test_the_fluxes_are_darcys(darcy_columns):
    """probe["q"] and probe["r"] against the 40-digit Darcy flux of the profile, inside flux_errors' bound (r[j] = q[j - 1] - q[j]:
    the two bounds and one rounding of the larger flux)."""
    worst = 0.0
    for c, th, zwt_m, par, hksat, pe, q, r, probe in darcy_columns:
        eq = flux_errors(c, zwt_m, par, hksat, th, pe, q)
        rows = N + 1 if len(pe) > N else N
        for i in range(N):
            err = abs(mp.mpf(probe["q"][i]) - q[i])
            assert err <= eq[i] * U, (i, float(err), eq[i] * U, float(q[i]))
            if eq[i]:
                worst = max(worst, float(err) / (eq[i] * U))
        for j in range(rows):
            lo, hi = (eq[j - 1] if j else 0.0), (eq[j] if j < N else 0.0)
            big = max(abs(float(q[j - 1])) if j else 0.0, abs(float(q[j])) if j < N else 0.0)
            assert abs(mp.mpf(probe["r"][j]) - r[j]) <= (lo + hi + 2 * big) * U, j
        assert max(abs(float(v)) for v in q) > 1.0e-9  # something flows
    print(f"largest |q - Darcy| relative to its bound: {worst:.3f}")
    assert worst > 1.0e-4  # the bound is not vacuous: within four decades of what is measured


def test_the_change_over_a_vanishing_step_tends_to_the_right_hand_side():
    """Without the probe: (liq_new - liq) / dt at dt = 1e-2 s and 1e-3 s against r[j] of the reference, in wet columns (s from 0.6:
    the implicit part, of first order in dt, stands clear of the rounding of liq / dt).  The error, the largest over the layers,
    falls to under a fifth from the longer to the shorter step (a tenth, were there no rounding)."""
    for theta, zwt_m, par, hksat in random_columns(9, 23, smin=0.6, smax=0.97):
        zwt_m = min(zwt_m, 3.6)
        c = build(theta, zwt_m, par, hksat)
        th = [mp.mpf(c["liq"][j]) / (mp.mpf(c["dz"][j]) * 1000) for j in range(N)]
        _, r = darcy(th, zwt_m, par, hksat)
        err = []
        for dt in (1.0e-2, 1.0e-3):
            o = hy.column(c, dt)
            err.append(max(abs((mp.mpf(o["liq"][j]) - mp.mpf(c["liq"][j])) / mp.mpf(dt) - r[j]) for j in range(N)))
        scale = max(abs(v) for v in r)
        assert err[0] < 1.0e-2 * scale, (float(err[0]), float(scale))
        assert err[1] < err[0] / 5, (float(err[0]), float(err[1]))


def test_the_linearisation_is_the_derivative_of_the_flux(darcy_columns):
    """probe["dq1"][i] and probe["dq2"][i] against mpmath.diff of the reference flux through interface i with respect to the water
    content of node i and of node i + 1, for the interfaces between two layers (there CLM's dhkdw is the exact derivative of the
    interface conductivity; at the interface to the aquifer node it is half of it, by CLM's own statement, and is not asserted).

    Bound: dq = -(-+ hk dsmpdw + num dhkdw) / den.  hk and dhkdw carry the conductivity's ((2 bsw + 3) 4 + 5) U, dsmpdw = -bsw smp /
    (s watsat) the potential's (5 bsw + 3) U and four more; num carries the absolute error of the head difference.  So the error is
    at most [(|hk dsmpdw| + |num dhkdw|) (8 bsw + 5 bsw' + 30) + |dhkdw| head] U / den, bsw' the other node's."""
    worst = 0.0
    for c, th, zwt_m, par, hksat, pe, q, r, probe in darcy_columns:
        e_smp, e_zq = potential_errors(c, zwt_m, par, pe)
        for i in range(N - 1):
            def flux(a, b_, i=i):
                t = list(th)
                t[i], t[i + 1] = a, b_
                s = (a + b_) / (mp.mpf(par["watsat"][i]) + mp.mpf(par["watsat"][i + 1]))
                k = mp.mpf(hksat[i]) * s ** (2 * mp.mpf(par["bsw"][i]) + 3)
                return -k * ((psi(b_, par, i + 1) - psi(a, par, i)) - (pe[i + 1] - pe[i])) / (ZMM[i + 1] - ZMM[i])

            want1 = mp.diff(flux, (th[i], th[i + 1]), (1, 0))
            want2 = mp.diff(flux, (th[i], th[i + 1]), (0, 1))
            den = float(ZMM[i + 1] - ZMM[i])
            s = (th[i] + th[i + 1]) / (mp.mpf(par["watsat"][i]) + mp.mpf(par["watsat"][i + 1]))
            hk = float(mp.mpf(hksat[i]) * s ** (2 * mp.mpf(par["bsw"][i]) + 3))
            dhk = hk * (2 * par["bsw"][i] + 3) / float(th[i] + th[i + 1])
            num = abs(float((psi(th[i + 1], par, i + 1) - psi(th[i], par, i)) - (pe[i + 1] - pe[i])))
            head = e_smp[i] + e_smp[i + 1] + e_zq[i] + e_zq[i + 1] + 3 * max(abs(float(pe[i])), abs(float(pe[i + 1])), e_smp[i] / 3, e_smp[i + 1] / 3)
            for got, want, node in ((probe["dq1"][i], want1, i), (probe["dq2"][i], want2, i + 1)):
                dpsi = par["bsw"][node] * abs(float(psi(th[node], par, node))) / float(th[node])
                bound = ((hk * dpsi + num * dhk) * (8 * par["bsw"][i] + 5 * par["bsw"][node] + 30) + dhk * head) * U / den
                err = float(abs(mp.mpf(got) - want))
                assert err <= bound, (i, node, err, bound, float(want))
                worst = max(worst, err / bound)
    print(f"largest |dq - d(flux)/d(theta)| relative to its bound: {worst:.3f}")
    assert worst > 1.0e-4


# The multiple of 2^-52 per row that bounds the residual of the Thomas solve relative to max |b| max |u|.  LU of a tridiagonal matrix
# without pivoting followed by the two substitutions solves (A + dA) u = r with |dA| <= (4 U + O(U^2)) |L| |U| (Higham, Accuracy and
# Stability of Numerical Algorithms, theorem 9.14), and |L| |U| <= 3 |A| where A is diagonally dominant or an M-matrix: a residual
# of at most 12 U |A| |u|, and a row of |A| sums to at most 3 max |b| where the diagonal dominates: 36 U = 18 * 2^-52, in every row
# on its own.  The rows of the soil water are dominant where the heads are near equilibrium; far from it the dhkdw terms can outweigh
# the diagonal and the factors grow, which the row count allows for.
RESIDUAL_MULTIPLE = 18.0


def residual(probe):
    """max_j |(A u - r)_j| in 40 digits / (max |b| max |u|)."""
    a, b, cc, r, u = ([mp.mpf(v) for v in probe[k]] for k in ("a", "b", "cc", "r", "u"))
    n = len(u)
    res = [abs((a[j] * u[j - 1] if j else 0) + b[j] * u[j] + (cc[j] * u[j + 1] if j < n - 1 else 0) - r[j]) for j in range(n)]
    scale = max(abs(v) for v in b) * max(abs(v) for v in u)
    return float(max(res) / scale) if scale else 0.0


def test_the_solve_leaves_a_residual_of_rounding_size(darcy_columns):
    bound = RESIDUAL_MULTIPLE * 2.0 ** -52 * (N + 1)
    worst = max(residual(p[8]) for p in darcy_columns)
    print(f"the unsaturated columns: largest residual {worst:.3e} (bound {bound:.3e})")
    assert 0.0 < worst <= bound
    for frost in (False, True):
        g = edge_columns(519, 5, frost=frost)  # three rounds of the tier's classes
        probes = []
        hy.step(g[0], g[1], DT, frost=g[2] if frost else None, probes=probes)
        fin = edge_finite(519)
        got = [residual(p) for i, p in enumerate(probes) if fin[i] and all(math.isfinite(v) for v in p["u"])]
        assert len(got) >= 140
        print(f"the edge tier's finite columns ({'frost' if frost else 'plain'}): largest residual {max(got):.3e}")
        assert max(got) <= bound


# ---- d. drainage and runoff --------------------------------------------------------------------------------------------------------
def test_runoff_and_drainage_are_their_closed_forms():
    """Nothing flows (hksat = 0): fsat = wtfact exp(-0.25 zwt); rsub_top = 10^(-6 i) rsub_top_max exp(-2.5 zwt) with i the
    thickness-weighted ice fraction of the layers from the one above the table's down; the water removed is rsub_top dt, out of the
    soil with the table inside the column and out of the aquifer with it below; and the table falls by rsub_top dt / (1000 sy) where
    the walk ends in the table's layer.

    Bounds: exp(x) carries (|x| + 2) U (its argument's rounding and its own); 10^x carries (|x| ln 10 (n + 3) + 2) U with n the
    number of layers summed into i; the products one U each.  The water removed is a difference of sums of ten terms: 24 U of the
    largest store.  sy = watsat (1 - t), t = (1 + 1000 zwt / sucsat)^(-1 / bsw), carries (6 t / (1 - t) + 4) U; the fall is a
    difference of two depths and carries 2 U zwt on top."""
    wtfact, rmax = 0.37, 2.0e-3
    worst = {}
    for zwt_m in (0.03, 0.2, 0.7, 1.9, 3.3, 5.0, 11.0):
        for icy in (False, True):
            c = column(zwt=zwt_m, hksat=0.0, wtfact=wtfact, rsub_top_max=rmax, sat=0.5)
            c["watsat"] = [0.45 + 0.02 * j for j in range(N)]
            c["sucsat"] = [80.0 + 15.0 * j for j in range(N)]
            c["bsw"] = [3.5 + 0.5 * j for j in range(N)]
            if icy:
                for j in range(3, N):
                    c["ice"][j] = (0.05 + 0.03 * j) * c["watsat"][j] * (c["dz"][j] * 917.0)
            o = hy.column(c, DT)
            z = mp.mpf(zwt_m)
            want = mp.mpf(wtfact) * mp.exp(-z / 4)
            assert abs(mp.mpf(o["fsat"]) - want) <= (0.25 * zwt_m + 3) * U * want
            jwt = hy._jwt(zwt_m, ZI)
            first = max(jwt - 1, 0)
            frac = [min(mp.mpf(1), mp.mpf(c["ice"][j]) / (mp.mpf(c["dz"][j]) * 917) / mp.mpf(c["watsat"][j])) for j in range(N)]
            thick = [mp.mpf(c["dz"][j]) for j in range(N)]
            ibar = sum(frac[j] * thick[j] for j in range(first, N)) / sum(thick[first:])
            rsub = 10 ** (-6 * ibar) * mp.mpf(rmax) * mp.exp(-mp.mpf("2.5") * z)
            tol = (6 * float(ibar) * math.log(10.0) * (N - first + 3) + 2 + 2.5 * zwt_m + 2 + 2) * U
            assert abs(mp.mpf(o["qflx_drain"]) - rsub) <= tol * rsub, (zwt_m, icy)
            worst["rsub_top"] = max(worst.get("rsub_top", 0.0), float(abs(mp.mpf(o["qflx_drain"]) - rsub) / rsub) / tol)
            assert o["qflx_rsub_sat"] == 0.0 and o["qcharge"] == 0.0 and o["qflx_surf"] == 0.0
            removed = (sum(mp.mpf(v) for v in c["liq"]) - sum(mp.mpf(v) for v in o["liq"])) + (mp.mpf(c["wa"]) - mp.mpf(o["wa"]))
            assert abs(removed - rsub * DT) <= 24 * U * max(max(c["liq"]), c["wa"]) + tol * float(rsub) * DT, (zwt_m, icy)
            k = min(jwt, N - 1)
            if jwt == N:
                assert o["liq"] == c["liq"] and o["wa"] <= c["wa"]  # (at 11 m the baseflow is under the rounding of wa)
            else:
                assert o["wa"] == c["wa"] and o["liq"][:jwt] == c["liq"][:jwt]
            t = (1 + 1000 * z / mp.mpf(c["sucsat"][k])) ** (-1 / mp.mpf(c["bsw"][k]))
            sy = max(mp.mpf("0.02"), mp.mpf(c["watsat"][k]) * (1 - t))
            fall = rsub * DT / (1000 * sy)
            if jwt == N or z + fall < mp.mpf(ZI[jwt + 1]):  # the walk ends in the table's layer
                got = mp.mpf(o["zwt"]) - z
                tol_f = (tol + (6 * float(t / (1 - t)) + 6) * U) * float(fall) + 4 * U * zwt_m
                assert abs(got - fall) <= tol_f, (zwt_m, icy, float(got), float(fall))
                worst["fall"] = max(worst.get("fall", 0.0), float(abs(got - fall)) / tol_f)
    print({k: round(v, 3) for k, v in worst.items()})
    assert worst["rsub_top"] > 0.0 and worst["fall"] > 0.0
