"""Floodplain inundation without a GPU (include/elmk.h "floodplain inundation"): mass and the inverse of the volume curve in exact
rational arithmetic, monotony across the breakpoints, the bits of the plain scheme where no water leaves the banks, the return of
floodplain water and the closed budget, the hydrograph of a storm with and without banks, every refusal of the check, the same check
of elmkernels_amd/csrc/elmk_maps.h through a stand-alone program (plain and under the address and undefined-behaviour sanitizers) with
its tables bit for bit, and the header's constants and the bindings."""
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from elmkernels_amd import _lib as L
from elmkernels_amd import routing as rt
from elmkernels_amd import state as st
from tests import inundation_cases as ic
from tests.support import ROOT, bits

U = 2.0 ** -53  # the unit roundoff of fp64
NAN, INF = float("nan"), float("inf")
F = Fraction


def _fsum(x):
    """The exact sum of finite doubles."""
    return sum((F(v) for v in np.asarray(x, dtype=np.float64).tolist()), F(0))


@pytest.fixture(scope="module")
def cells():
    area, p, rdepth, eprof, volr, wf = ic.random_cells(20000, 2201)
    tab = rt.inundation_tables(area, p, rdepth, eprof)
    return area, p, tab, volr, wf, rt.inundation_exchange(volr, wf, tab, area)


# ---- mass ------------------------------------------------------------------------------------------------------------------------------
def test_the_exchange_keeps_the_water(cells):
    """VOLR + WF after the exchange against W = fl(v + WF), in exact arithmetic, on 20 000 random cells.  The count: I2 stores W and
    0.0, no rounding; I4 stores vc2 and fl(W - vc2), one rounding, of a difference that lies in [0, W] because vc2 is clamped to W and
    is not negative: |VOLR + WF - W| <= u (W - vc2) <= u W, half an ulp of W.  An untouched cell keeps both values.  WF is never
    negative, FLOOD_FRAC stays in [0, 1), and a second exchange moves VOLR by at most 2 ulp (measured: 2)."""
    area, p, tab, volr, wf, (v1, wf1, h, fr) = cells
    path = ic.path_census(volr, wf, tab)
    assert set(np.unique(path)) == set(range(13))  # every path is among the cells
    worst = 0.0
    for c in range(volr.size):
        w = float(volr[c] + wf[c])
        got = F(float(v1[c])) + F(float(wf1[c]))
        if path[c] == 0:
            assert got == F(float(volr[c])) + F(float(wf[c])) and v1[c] == volr[c] and wf1[c] == wf[c]
        else:
            worst = max(worst, float(abs(got - F(w)) / F(w)))
            assert abs(got - F(w)) <= F(U) * F(w), c
    print(f"mass: worst |VOLR + WF - W| / W = {worst:.3e} (u = {U:.3e})")
    assert (wf1 >= 0.0).all() and (fr >= 0.0).all() and (fr < 1.0).all() and (h >= 0.0).all()
    assert (fr[area == 0.0] == 0.0).all() and (area == 0.0).sum() > 100
    v2 = rt.inundation_exchange(v1, wf1, tab, area)[0]
    moved = np.abs(v2 - v1) / np.spacing(np.maximum(v1, v2))
    print(f"a second exchange moves VOLR by at most {moved.max():.1f} ulp")
    assert moved.max() <= 2.0


# ---- the inverse -----------------------------------------------------------------------------------------------------------------------
def _volume(h, c, tab, x):
    """The volume over the bank top at level h in cell c, exactly: VB_k + S_k d + M_k d^2 / 2 in the segment X lies in, linear above
    the profile."""
    vb, e, s, m = (tab[k][:, c] for k in ("VB", "E", "S", "M"))
    if x >= vb[10]:
        return F(float(vb[10])) + F(float(s[10])) * (F(h) - F(float(e[10])))
    k = max(j for j in range(10) if x >= vb[j])
    d = F(h) - F(float(e[k]))
    return F(float(vb[k])) + F(float(s[k])) * d + F(float(m[k])) * d * d / 2


def test_the_level_inverts_the_volume_curve(cells):
    """The volume of h, evaluated with fractions.Fraction from the statement's tables, against X = W - VC on the first 3 000 flooded
    cells.  Measured on these inputs: 6.2e-16 relative at the worst; the bound is four times that, 2.5e-15.  The margin covers other
    seeds, not other algorithms: the naive root (-S + sqrt(S^2 + 2 M r)) / M cancels and misses the bound, which the
    test shows on the same cells."""
    area, p, tab, volr, wf, (v1, wf1, h, fr) = cells
    bound = 4 * 6.2e-16
    w = volr + wf
    flooded = np.nonzero(ic.path_census(volr, wf, tab) >= 2)[0][:3000]
    assert flooded.size == 3000
    worst = naive_worst = 0.0
    for c in flooded:
        x = float(w[c] - tab["VC"][c])
        worst = max(worst, float(abs(_volume(float(h[c]), c, tab, x) - F(x)) / F(x)))
        if x < tab["VB"][10, c] and tab["AF"][c] > 0.0:
            k = max(j for j in range(10) if x >= tab["VB"][j, c])
            s, m, r = tab["S"][k, c], tab["M"][k, c], x - tab["VB"][k, c]
            hn = tab["E"][k, c] + (np.sqrt(s * s + (2.0 * m) * r) - s) / m
            naive_worst = max(naive_worst, float(abs(_volume(float(hn), c, tab, x) - F(x)) / F(x)))
    print(f"inverse: worst relative difference {worst:.3e} (bound {bound:.3e}); the cancelling root: {naive_worst:.3e}")
    assert worst <= bound
    assert naive_worst > bound


# ---- monotony --------------------------------------------------------------------------------------------------------------------------
def test_level_and_fraction_rise_with_the_water(cells):
    """With VC taken as 0.0, so that X = W exactly: at X = VB_k the level is E_k and the fraction AF f_k / area, bit for bit, and over
    W ascending through every breakpoint neither h nor FLOOD_FRAC falls.  The points: each VB_k, VB_k (1 -+ j 2^-40) for j = 1, 2, 3,
    and seven points inside every segment and above the profile.  The spacing comes from the rounding of I3: d carries about five
    roundings (4 u relative and more where it is clipped), so two levels are told apart for certain only when they differ by more than
    some 10 u h.  A step of 2^-40 in X moves h by 2^-40 X / (S h), and X / (S h) is at least 0.05 on any profile (all of the rise in
    the first tenth: X = 0.05 AF E against S h = k 0.1 AF E), that is by 4e-14 h, four hundred roundings.  Between neighbouring
    doubles the order is not kept: measured on these cells, h steps back by one ulp inside a segment, and at the end of a segment
    f_k + 0.1 lies up to 2 ulp above f_{k+1} at 182 of 30 000 breakpoints."""
    area, p, tab, volr, wf, _ = cells
    step = 2.0 ** -40
    for c in range(0, 900, 3):
        vb = tab["VB"][:, c]
        ws = set()
        for k in range(11):
            if k:
                ws.update(float(vb[k] * (1.0 + j * step)) for j in (-3, -2, -1, 0, 1, 2, 3))
            hi = vb[k + 1] if k < 10 else 3.0 * vb[10]
            ws.update(float(vb[k] + t * (hi - vb[k])) for t in (1.0e-9, 1.0e-6, 0.01, 0.3, 0.5, 0.9, 0.999999))
        ws = np.array(sorted(ws))
        one = {k: v if k == "F" else np.repeat(v[:, c:c + 1], ws.size, axis=1) if v.ndim == 2 else np.repeat(v[c], ws.size) for k, v in tab.items()}
        one["VC"] = np.zeros(ws.size)
        _, _, h, fr = rt.inundation_exchange(ws, np.zeros(ws.size), one, np.repeat(area[c], ws.size))
        assert (np.diff(h) >= 0.0).all(), (c, ws[1:][np.diff(h) < 0.0][:3])
        assert (np.diff(fr) >= 0.0).all(), (c, ws[1:][np.diff(fr) < 0.0][:3])
        assert (np.diff(h) > 0.0).sum() >= ws.size - 2 - 60 * (tab["AF"][c] == 0.0)
        for k in range(1, 11):
            i = int(np.nonzero(ws == vb[k])[0][0])
            assert h[i] == tab["E"][k, c], (c, k)
            assert fr[i] == ((tab["AF"][c] * tab["F"][k]) / area[c] if area[c] > 0.0 else 0.0), (c, k)


# ---- the plain scheme's bits ---------------------------------------------------------------------------------------------------------
def test_inside_its_banks_the_river_keeps_the_plain_schemes_bits():
    """WF = 0 and VOLR <= VC throughout (banks of 1e4 m): kinematic_call(flood=...) returns the bits of kinematic_call without it on
    all seven rows (QIN and QSUR are inputs here), over five chained calls with the edge values that stay inside any banks, and WF
    and the diagnostics stay +0.0."""
    n = 257
    ddist, area, p, volr, wh, wt = ic.cell_values(n, 40 + n)
    rng = np.random.default_rng(5)
    qin = (rng.uniform(-1.0e-5, 4.0e-5, n) * 0.001) * area
    qsur = qin * rng.uniform(0.0, 1.0, n)
    up = rt.upstream_map(ic.networks(n, 50 + n)["forest"])
    eprof = np.repeat((0.5 * np.arange(11))[:, None], n, axis=1)
    tab = rt.inundation_tables(area, p, np.full(n, 1.0e4), eprof)
    volr, wh, wt = (np.where((x == 1e300) | (x == INF), 7.0, x) for x in (volr, wh, wt))  # (these two leave any banks)
    a, b, wf = (wh, wt, volr), (wh, wt, volr), np.zeros(n)
    qsum_a = qsum_b = np.zeros(n)
    for _ in range(5):
        with np.errstate(all="ignore"):
            assert not (b[2] > tab["VC"]).any()
        a = rt.kinematic_call(*a[:3], qin, qsur, area, p, up, 1800.0, 3)
        b = rt.kinematic_call(*b[:3], qin, qsur, area, p, up, 1800.0, 3, flood=(tab, wf))
        with np.errstate(all="ignore"):
            qsum_a, qsum_b = rt._canon(qsum_a + a[3]), rt._canon(qsum_b + b[3])
        for x, y in zip(a + (qsum_a,), b[:4] + (qsum_b,)):
            assert bits(x) == bits(y)
        wf = b[4]
        assert not wf.any() and not np.signbit(wf).any() and not b[5].any() and not b[6].any()
    assert np.isnan(b[2]).any() and (b[2] < 0.0).any() and (b[2] > 1.0e5).any()


# ---- the return of water, and the budget -----------------------------------------------------------------------------------------------
def _closed(before, after, qin, qout, down, dt, nsub):
    """The residual of I7 over one call in exact arithmetic and its bound.  before, after: (WH, WT, VOLR, WF).  The bound is the
    kinematic scheme's (tests/test_routing_kinematic_host.py: 17 nsub SC + 5 dt Q + (nsub + 1) nsub SC + dt (SQ + SO), SC the storages
    at the call's start plus dt Q, now with WF among them) plus the exchange's two roundings per cell and sub-step, W = fl(v + WF) and
    WF = fl(W - vc2), each at most u times what the cell holds: 2 nsub SC more."""
    so = _fsum(qout[down < 0])
    res = sum(_fsum(x) for x in after) - sum(_fsum(x) for x in before) - F(dt) * (_fsum(qin) - so)
    q = 2.0 * float(np.abs(qin).sum())
    sc = float(sum(np.abs(x).sum() for x in before)) + dt * q
    return abs(res), 1.01 * U * ((19 + (nsub + 1)) * nsub * sc + 5 * dt * q + dt * (float(np.abs(qin).sum()) + float(so)))


def test_a_flooded_cell_hands_its_water_back():
    """A chain of eight flooded cells whose inflow has stopped: WF falls call by call to exactly 0.0 in every cell, FLOOD_DEPTH and
    FLOOD_FRAC with it, and the I7 budget closes in every call inside its counted bound."""
    down, area, p, rdepth, eprof = ic.storm_chain()
    n, dt, nsub = down.size, 1800.0, 4
    tab = rt.inundation_tables(area, p, rdepth, eprof)
    up = rt.upstream_map(down)
    wh = wt = np.zeros(n)
    volr, wf = tab["VC"] * 1.2, np.full(n, 3.0e6)
    zero = np.zeros(n)
    first = rt.inundation_exchange(volr, wf, tab, area)
    assert (first[1] > 0.0).all() and (first[2] > 0.0).all() and (first[3] > 0.0).all()
    total, total_bound, ncalls, last_wf = F(0), 0.0, 0, wf.sum()
    while wf.any():
        out = rt.kinematic_call(wh, wt, volr, zero, zero, area, p, up, dt, nsub, flood=(tab, wf))
        res, bound = _closed((wh, wt, volr, wf), (out[0], out[1], out[2], out[4]), zero, out[3], down, dt, nsub)
        assert res <= bound, (ncalls, float(res), bound)
        total, total_bound = total + res, total_bound + bound
        wh, wt, volr, wf = out[0], out[1], out[2], out[4]
        assert (wf >= 0.0).all() and ((out[5] > 0.0) == (wf > 0.0)).all() and ((out[6] > 0.0) == (wf > 0.0)).all()
        assert wf.sum() <= last_wf  # (no inflow from the land: the floodplains only drain)
        last_wf = wf.sum()
        ncalls += 1
        assert ncalls < 5000
    print(f"the floodplains were dry after {ncalls} calls; summed residual {float(total):.3e} m3, summed bound {total_bound:.3e}")
    assert ncalls > 10 and not wf.any() and not np.signbit(wf).any() and (volr <= tab["VC"]).all()


# ---- the hydrograph ---------------------------------------------------------------------------------------------------------------------
def test_banks_lower_and_delay_the_flood_peak():
    """The storm of examples/kinematic_routing_demo.cc on the eight-cell chain, made heavy enough (40 mm/h for six hours, all of it
    runoff, half of it over the surface) that the channel without banks stands above RDEPTH in at least half the cells: with banks the
    outlet's peak QOUT is lower and not earlier, and total outflow plus remaining storage agree between the two runs inside the summed
    counted bounds."""
    down, area, p, rdepth, eprof = ic.storm_chain()
    n, dt, nsub, nsteps, storm_steps = down.size, 1800.0, 4, 96, 12
    tab = rt.inundation_tables(area, p, rdepth, eprof)
    up = rt.upstream_map(down)
    rain = 40.0 / 3600.0  # mm/s
    runs = {}
    for banks in (False, True):
        wh = wt = volr = np.zeros(n)
        wf = np.zeros(n)
        q, deepest, flooded, out_volume, bound = [], np.zeros(n), np.zeros(n), F(0), 0.0
        for s in range(nsteps):
            qin = np.full(n, ((rain if s < storm_steps else 0.0) * 0.001) * 1.0e8)
            qsur = 0.5 * qin
            before = (wh, wt, volr, wf)
            if banks:
                wh, wt, volr, qout, wf, depth, frac = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub, flood=(tab, wf))
                flooded = np.maximum(flooded, frac)
            else:
                wh, wt, volr, qout = rt.kinematic_call(wh, wt, volr, qin, qsur, area, p, up, dt, nsub)
            bound += _closed(before, (wh, wt, volr, wf), qin, qout, down, dt, nsub)[1]
            deepest = np.maximum(deepest, (volr / p[rt.RLEN]) / p[rt.RWIDTH])
            q.append(qout[-1])
            out_volume += F(float(qout[-1])) * F(dt)
        runs[banks] = (np.array(q), deepest, out_volume + _fsum(wh) + _fsum(wt) + _fsum(volr) + _fsum(wf), bound, flooded)
    plain, flood = runs[False], runs[True]
    assert (plain[1] > rdepth).sum() >= n // 2  # the bankless channel stands above the bank height in at least half the cells
    assert (flood[4] > 0.0).sum() >= n // 2
    print(f"outlet peak without banks {plain[0].max():.4e} m3/s at step {plain[0].argmax()}, with banks {flood[0].max():.4e} at step "
          f"{flood[0].argmax()}; deepest bankless channel {plain[1].max():.2f} m over banks of {rdepth[0]} m; largest flooded fraction "
          f"{flood[4].max():.3f}; totals differ by {float(abs(plain[2] - flood[2])):.3e} m3, bound {plain[3] + flood[3]:.3e}")
    assert flood[0].max() < plain[0].max() and flood[0].argmax() >= plain[0].argmax()
    assert abs(plain[2] - flood[2]) <= plain[3] + flood[3]


# ---- the checks --------------------------------------------------------------------------------------------------------------------------
def test_check_inundation_refuses_what_the_statement_excludes():
    n = 6
    good_r = np.full(n, 2.0)
    good_e = np.repeat((0.25 * np.arange(11))[:, None], n, axis=1)
    rt.check_inundation(good_r, good_e)
    for c, bad in enumerate((0.0, -0.0, -1.0, NAN, INF, -INF)):
        r = good_r.copy()
        r[c] = bad
        with pytest.raises(ValueError, match="^" + re.escape(rt.e_cell(rt.E_RDEPTH, c)) + "$"):
            rt.check_inundation(r, good_e)
    for k in range(rt.NPROF):
        for bad in (NAN, INF, -INF):
            e = good_e.copy()
            e[k, k % n] = bad
            with pytest.raises(ValueError, match="^" + re.escape(rt.e_cell(rt.E_EPROF_FINITE, k % n)) + "$"):
                rt.check_inundation(good_r, e)
    for bad in (1.0e-3, -1.0e-3, 5e-324):
        e = good_e.copy()
        e[0, 4] = bad
        with pytest.raises(ValueError, match="^" + re.escape(rt.e_cell(rt.E_EPROF_ZERO, 4)) + "$"):
            rt.check_inundation(good_r, e)
    e = good_e.copy()
    e[0, 4] = -0.0
    rt.check_inundation(good_r, e)
    for k in range(1, rt.NPROF):
        for step in (0.0, -0.5):
            e = good_e.copy()
            e[k, k % n] = e[k - 1, k % n] + step
            with pytest.raises(ValueError, match="^" + re.escape(rt.e_cell(rt.E_EPROF_ORDER, k % n)) + "$"):
                rt.check_inundation(good_r, e)
    # the first offending cell; rdepth before any of the profile; inside a cell finite, then the first entry, then the order
    e = good_e.copy()
    e[5, 4], e[9, 2] = NAN, 0.0
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_EPROF_ORDER, 2))):
        rt.check_inundation(good_r, e)
    r = good_r.copy()
    r[4] = 0.0
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_RDEPTH, 4))):
        rt.check_inundation(r, e)
    e = good_e.copy()
    e[0, 1], e[3, 1], e[7, 1] = 1.0, 0.1, NAN
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_EPROF_FINITE, 1))):
        rt.check_inundation(good_r, e)
    e[7, 1] = good_e[7, 1]
    with pytest.raises(ValueError, match=re.escape(rt.e_cell(rt.E_EPROF_ZERO, 1))):
        rt.check_inundation(good_r, e)
    for shape in ((10, n), (11, n + 1), (11 * n,)):
        with pytest.raises(ValueError, match="eprof must be"):
            rt.check_inundation(good_r, np.zeros(shape))
    with pytest.raises(ValueError, match=re.escape(rt.E_EPROF_ORDER)):
        rt.inundation_tables(np.ones(n), np.ones((11, n)), good_r, np.zeros((11, n)))


# ---- the same check in C: tests/c/inundation_checks.cc ---------------------------------------------------------------------------------
BADS = ((0.0, "0"), (-0.0, "-0"), (-1.0, "negative"), (NAN, "NaN"), (INF, "inf"), (-INF, "-inf"))


def c_valid(n):
    """The program's accepted inputs, by the same operations."""
    rdepth = np.array([0.5 + 0.37 * float(c % 7) for c in range(n)])
    area = np.array([0.0 if c == 1 else 1.0e8 * (1.0 + 0.011 * float(c % 13)) for c in range(n)])
    p = np.ones((rt.NPARAM, n))
    p[rt.RLEN] = [2.0e4 * (1.0 + 0.013 * float((c * 7) % 11)) for c in range(n)]
    p[rt.RWIDTH] = [1.0e4 if c == 2 else 100.0 * (1.0 + 0.017 * float((c * 3) % 5)) for c in range(n)]
    eprof = np.zeros((rt.NPROF, n))
    for k in range(1, rt.NPROF):
        for c in range(n):
            eprof[k, c] = eprof[k - 1, c] + 0.013 * float(k + c % 3) + 0.001
    return rdepth, eprof, area, p


def _text(rdepth, eprof, n=5, show=False):
    """What the program prints for these inputs, from the restatement."""
    try:
        rt.check_inundation(rdepth, eprof)
    except ValueError as e:
        return str(e)
    if not show:
        return "ok"
    _, _, area, p = c_valid(n)
    t = rt.inundation_tables(area, p, rdepth, eprof)
    rows = [t["VC"], t["ACHN"], t["AF"]] + list(t["E"]) + list(t["VB"])
    return "ok " + " ".join(float(v).hex() for r in rows for v in r)


def expected():
    n = 5
    r0, e0, _, _ = c_valid(n)
    out = [("ncells 0", rt.E_NCELLS), ("ncells 2^31", rt.E_NCELLS), ("null rdepth", "null argument"), ("null eprof", "null argument"),
           ("null area", "null argument")]
    for b, (bad, name) in enumerate(BADS):
        r = r0.copy()
        r[b % n] = bad
        out.append((f"RDEPTH {name}", _text(r, e0)))
    for k in range(rt.NPROF):
        for b in range(3, 6):
            e = e0.copy()
            e[k, (k + b) % n] = BADS[b][0]
            out.append((f"EPROF[{k}] {BADS[b][1]}", _text(r0, e)))
    for bad, name in ((1.0e-3, "positive"), (-1.0e-3, "negative"), (-0.0, "-0")):
        e = e0.copy()
        e[0, 3] = bad
        out.append((f"EPROF[0] {name}", _text(r0, e)))
    for k in range(1, rt.NPROF):
        for step, name in ((0.0, "flat"), (-0.5, "falling")):
            e = e0.copy()
            e[k, k % n] = e[k - 1, k % n] + step
            out.append((f"EPROF[{k}] {name}", _text(r0, e)))
    e = e0.copy()
    e[5, 4], e[9, 2] = NAN, 0.0
    out.append(("falling in cell 2 and NaN in cell 4", _text(r0, e)))
    r = r0.copy()
    r[4] = 0.0
    out.append(("... and bad RDEPTH in cell 4", _text(r, e)))
    r, e = r0.copy(), e0.copy()
    r[0], e[10, 1] = 5e-324, 1.7e308
    out.append(("denormal RDEPTH and huge EPROF[10]", _text(r, e)))
    out.append(("valid", _text(r0, e0, show=True)))
    r1, e1, _, _ = c_valid(1)
    out.append(("one cell", _text(r1, e1, n=1, show=True)))
    return out + [("sixty-four cells", "ok"), ("sixty-five cells", "ok"), ("ld 0", "ok size=125")]


def _build_and_run(tmp, sanitized):
    exe = str(tmp / ("inundation_checks_san" if sanitized else "inundation_checks"))
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "elmkernels_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "inundation_checks.cc"), "-o", exe]
    if sanitized:
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return None, r.stderr.decode()
    # stand-alone: the program has its own main and nothing of it is loaded into Python.  (Leak detection needs ptrace, which a
    # container may deny.)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, r.stderr.decode()
    return r.stdout.decode().splitlines(), ""


def _normal(lines):
    """(case, text) with every hexadecimal double in Python's spelling."""
    out = []
    for s in lines:
        name, text = s.split(": ", 1)
        out.append((name, " ".join(float.fromhex(w).hex() if w.startswith(("0x", "-0x")) else w for w in text.split(" "))))
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("inundation_checks")


def test_every_case_returns_the_entry_points_message_and_the_statements_tables(tmp):
    lines, err = _build_and_run(tmp, False)
    assert lines is not None, err
    got, want = _normal(lines), expected()
    assert [g[0] for g in got] == [w[0] for w in want]
    for g, w in zip(got, want):
        assert g == w, g[0]
    assert sum(w[1].startswith("ok") for w in want) == 7 and any("at cell 4" in w[1] for w in want)


def test_the_same_program_under_the_sanitizers(tmp):
    """-fsanitize=address,undefined, run stand-alone: an out-of-range read of the inputs or write of the tables ends the program."""
    lines, err = _build_and_run(tmp, True)
    if lines is None:
        pytest.fail("the host compiler does not link the sanitizers' static runtimes here:\n" + err[-400:])
    assert _normal(lines) == expected()


# ---- the budget, the header and the bindings -------------------------------------------------------------------------------------------
def test_the_budget_is_the_reductions_sum():
    from elmkernels_amd import diagnostics

    wf = np.random.default_rng(3).uniform(0.0, 1.0e7, 1001)
    got = rt.inundation_budget(wf)
    assert got.shape == (1,) and got[0] == diagnostics.reduce_min_max_sum(wf)[2]


def test_the_cost_tool_imports_without_device_or_library(tmp_path):
    """tests/tools/cost_routing_inundation.py imports without a device and without the built library, as tests/test_cost_tools_host.py
    asks of the *_cost.py tools, takes its protocol from costlib and its series length from the tool it is built on."""
    import sys

    tools = os.path.join(ROOT, "tests", "tools")
    src = open(os.path.join(tools, "cost_routing_inundation.py")).read()
    assert "import costlib as CL" in src and "perf_counter" not in src
    code = ("import sys, importlib\nsys.path.insert(0, sys.argv[1])\nm = importlib.import_module('cost_routing_inundation')\n"
            "r, e = m.banks(20, 'tenth')\nprint('imported', m.CALLS == m.CR.CALLS, e.shape, int((r < 1.0).sum()))\n")
    env = dict(os.environ, ELMK_LIBRARY=str(tmp_path / "no_such_libelmk.so"), HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, tools], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "imported True (11, 20) 2", r.stderr[-2000:]


ENTRY_POINTS = ("enable", "init", "budget", "clear")


def test_header_constants_and_bindings():
    h = open(os.path.join(ROOT, "include", "elmk.h")).read()
    assert "/* ---- floodplain inundation ----" in h
    assert h.index("/* ---- kinematic-wave routing ----") < h.index("/* ---- floodplain inundation ----") < h.index("/* ---- feature rows")
    assert "enum { ELMK_ROUTE_WF = 7, ELMK_ROUTE_FLOOD_DEPTH = 8, ELMK_ROUTE_FLOOD_FRAC = 9 };" in h and "#define ELMK_FP_NPROF 11" in h
    assert (rt.WF, rt.FLOOD_DEPTH, rt.FLOOD_FRAC) == (st.ROUTE_WF, st.ROUTE_FLOOD_DEPTH, st.ROUTE_FLOOD_FRAC) == (7, 8, 9)
    assert rt.NPROF == st.ROUTE_FP_NPROF == 11
    for name in ENTRY_POINTS:
        assert re.search(rf"^int elmk_routing_inundation_{name}\(", h, re.M) and f"elmk_routing_inundation_{name}" in L.SIGNATURES, name
        assert hasattr(st.ELMState, "routing_inundation_" + name)
    for k in range(9):
        assert f" I{k}." in h
    hpp = open(os.path.join(ROOT, "include", "elmk_interface.hpp")).read()
    for name in ENTRY_POINTS:
        assert f"elmk_routing_inundation_{name}(" in hpp, name
    # the kernel: a template parameter on the existing sub-step, no hint and no fence
    k = open(os.path.join(ROOT, "elmkernels_amd", "csrc", "k_routing.hip")).read()
    sub_step = "template <int NPAD, bool FIRST, bool LAST, bool FLOOD, bool DAM = false, bool HEAT = false>\n__global__ __launch_bounds__(256) void k_kinematic_step("
    assert sub_step in k and "nontemporal_" not in k and "__threadfence" not in k
