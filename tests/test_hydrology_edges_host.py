"""The edge tier of the soil hydrology on the host (tests/hydrology_cases.py: edge_columns) and the select census of the restatement
(tests/hydrology_sites.py): every `_min` / `_max` of hydrology.column() and hydrology._sy - a select in k_soil_hydrology - returns each
of its operands in some column of the generators plus the edge tier, apart from the sites listed in EXEMPT with the reason why no
input can flip them; every walk over the layers crosses two layer boundaries in some column and runs off the end of the layers in
another; every input is poisoned with NaN, +Inf and -Inf in a column of its own; and the host follows IEEE through all of it.

`pytest -s` prints the census."""
import numpy as np
import pytest

from elmkernels_amd import hydrology as hy
from tests import hydrology_sites as HS
from tests.hydrology_cases import (DT, EDGE_CLASS_NAMES, POISONED_FIELDS, POISONED_ROWS, POISONS, SOIL_FIELDS, edge_class_of, edge_columns,
                                   edge_finite, generated, generated_frost)

N = hy.N
NCOL, SEED = 1001, 5
DTS = (1.0, DT, 86400.0)
WALKS = ("E_rise", "E_fall", "F_drain", "FA_remove", "FB_remove")

# The sites that stay one-sided: (text of the statement, function, ordinal on the line, reason).  At most six; a site beyond this list
# means that inputs are missing from the edge tier.
EXEMPT = (
    ("ql = _max(0.0, _min(qt, sy * (zwt - zi[j]) * 1.0e3))", "_max", 0,
     "E's rising walk runs only where qt > 0, and over the layers j <= jwt, for which zwt > zi[j] (jwt is the first layer whose bottom "
     "is at or below zwt; sy >= 0.02): the inner minimum is positive, or it is qt itself where the product is NaN (b < a is false), so "
     "0.0 is never the larger.  zwt == zi[0] == 0 gives a product of +0, but there the recharge is smp[0] - zq[0] <= 0 and the walk "
     "does not run; and then both operands would be the same +0."),
    ("xs = _max(xs - take, 0.0)", "_max", 0,
     "take = _min(avail, xs) is xs or something smaller, so xs - take >= 0 whenever it is a number, and the statement runs only under "
     "xs > 0, which a NaN fails; a NaN avail makes take NaN and the first operand NaN, for which a < b is false as well."),
)
# The sites that return both operands, but one of them only where an operand is not finite: with these, the census counted over
# finite operands alone.  Together with EXEMPT still no more than six.
FINITE_EXEMPT = (
    ("ve = _min(watsat[j], _max(ve, 0.0))", "_max", 0,
     "the layer mean of the equilibrium profile: a positive factor times a difference of powers whose sign b1 = 1 - 1 / bsw turns "
     "together with the factor's; negative only where watsat or sucsat is -Inf"),
    ("zq[j] = _max(SMPMIN", "_max", 1,
     "ve / watsat falls under the 1 % clamp only where 1 + (zwt - z) / sucsat exceeds 100^bsw, and -sucsat * 100^bsw reaches SMPMIN only "
     "where that product exceeds 1e8: a water table more than 1e5 m down (zwt is kept at or under 80 m by F); sucsat = +Inf does it"),
    ("ve = _min(watsat[L], _max(ve, 0.0))", "_max", 0, "as in the layers, for the aquifer node"),
    ("zq[N] = _max(SMPMIN", "_max", 1, "as in the layers, for the aquifer node"),
)
assert len(EXEMPT) + len(FINITE_EXEMPT) <= 6


def _run(make, dts, census, walks=None, **kw):
    for frost in (False, True):
        g = make(frost, **kw)
        for dt in dts:
            probes = []
            with HS.recording(census):
                hy.step(g[0], g[1], dt, frost=g[2] if frost else None, probes=probes)
            if walks is not None:
                fin = edge_finite(len(probes))
                for i, p in enumerate(probes):
                    if fin[i]:
                        for w, (visited, ended) in p["walks"].items():
                            walks.setdefault(w, []).append((visited, ended))


def _generators(frost):
    return generated_frost(NCOL, 77) if frost else generated(NCOL, 77)


def _edges(frost, skip=()):
    return edge_columns(NCOL, SEED, frost=frost, skip=skip)


def census_of(skip=()):
    """-> (the census of the generators alone, of the generators plus the edge tier, the walks of the tier's finite columns)."""
    before = HS.Census()
    _run(_generators, (DT,), before)
    both = HS.Census()
    both.sites = {k: list(v) for k, v in before.sites.items()}
    walks = {}
    _run(_edges, DTS, both, walks, skip=skip)
    return before, both, walks


@pytest.fixture(scope="module")
def census():
    return census_of()


def exempt_sites(which=EXEMPT):
    return {(HS.line_of(text), fn, k) for text, fn, k, _ in which}


def test_every_static_site_is_seen(census):
    """The `ast` count of _min / _max calls per line of column() (nested functions included) and _sy equals the number of distinct
    bytecode offsets seen on that line at run time: no site is missing from the census and none is counted twice."""
    _, both, _ = census
    static = HS.static_sites()
    seen = {}
    for (line, fn, _k) in both.by_site():
        seen[(line, fn)] = seen.get((line, fn), 0) + 1
    assert seen == static
    assert sum(static.values()) == 51


def test_every_select_returns_both_operands(census):
    before, both, _ = census
    print("the generators alone: " + before.report().splitlines()[0])
    print("with the edge tier:   " + both.report())
    assert len(before.one_sided()) == 15  # what the tier set out from
    left = set(both.one_sided())
    assert left == exempt_sites(), (sorted(left - exempt_sites()), sorted(exempt_sites() - left))
    left = set(both.one_sided(finite=True))
    want = exempt_sites() | exempt_sites(FINITE_EXEMPT)
    assert left == want, (sorted(left - want), sorted(want - left))
    # non-finite operands reach the selects
    assert sum(1 for v in both.by_site().values() if v[2]) >= 40 and not any(v[2] for v in before.by_site().values())


def test_every_walk_crosses_layers_and_runs_out(census):
    """Per walk over the layers (E rises, E falls, F drains through the soil, F' removal A and B), in the finite columns of the tier:
    some column visits at least three layers, that is crosses two layer boundaries, and some column runs off the end of the walk -
    the surface, or the bottom of the last layer - with a remainder left."""
    _, _, walks = census
    for w in WALKS:
        got = walks.get(w, [])
        print(w, len(got), "walks,", sum(1 for v, _ in got if v >= 3), "over three layers or more,", sum(1 for _, e in got if e), "ran out")
        assert any(v >= 3 for v, _ in got), w
        assert any(e for _, e in got), w


@pytest.mark.parametrize("frost", [False, True], ids=["plain", "frost"])
def test_the_tier_holds_what_it_says(frost):
    """Against the generator's columns of the same seed: every column of the non-finite tier holds exactly one non-finite input, the
    one its class names, and NaN, +Inf and -Inf each sit in a column of their own in every float field the stage reads, every
    parameter and state row (ZWT .. RSUB_TOP_MAX), t_soisno and Q_PERCH_MAX.  The named finite edges are where the classes put them."""
    g = edge_columns(NCOL, SEED, frost=frost)
    cols, rows, fr = g[0], g[1], (g[2] if frost else None)
    cls = edge_class_of(NCOL)
    names = [EDGE_CLASS_NAMES[k] for k in cls]
    s0 = hy.NLEVSNO

    def nonfinite(i):
        out = []
        for k in POISONED_FIELDS:
            a = np.asarray(cols[k][i], dtype=np.float64).reshape(-1)
            out += [(k, float(v)) for v in a[~np.isfinite(a)]]
        out += [(f"row {w}", float(rows[w, i])) for w in range(hy.NROWS) if not np.isfinite(rows[w, i])]
        if fr is not None:
            out += [("q_perch_max", float(fr[w, i])) for w in range(hy.FROST_NROWS) if not np.isfinite(fr[w, i])]
        return out

    want = set()
    for v in POISONS:
        want |= {(k, repr(v)) for k in POISONED_FIELDS} | {(f"row {w}", repr(v)) for w in POISONED_ROWS}
        if frost:
            want.add(("q_perch_max", repr(v)))
    got = set()
    for i in range(NCOL):
        nf = nonfinite(i)
        if edge_finite(NCOL)[i]:
            assert not nf, (i, names[i], nf)
            continue
        if names[i].startswith("dz=0") or (names[i].startswith("q_perch_max=") and not frost):
            assert not nf
            continue
        assert len(nf) == 1, (i, names[i], nf)
        key, v = nf[0]
        if names[i].startswith("table below"):
            assert key in ("watsat", "sucsat", "bsw") and rows[hy.ZWT, i] == 8.0
            continue
        assert names[i] == f"{key}={v}", (i, names[i], nf)
        got.add((key, repr(v)))
    assert got == want, want - got
    assert len(POISONED_FIELDS) == len(hy.READS) and POISONED_ROWS == tuple(range(16)) and set(SOIL_FIELDS) < set(hy.READS)
    # the finite edges, where a value says it all
    at = {name: np.flatnonzero(np.array(names) == name) for name in EDGE_CLASS_NAMES}
    for name, w, v in (("zwt=0", hy.ZWT, 0.0), ("zwt=1e-9", hy.ZWT, 1.0e-9), ("zwt=80", hy.ZWT, 80.0), ("zwt=100", hy.ZWT, 100.0),
                       ("wa=0", hy.WA, 0.0), ("wa=5000", hy.WA, 5000.0), ("wa>5000", hy.WA, 5500.0), ("rsub_top_max=0", hy.RSUB_TOP_MAX, 0.0)):
        assert at[name].size >= 5 and (rows[w, at[name]] == v).all(), name
    for j in range(N):
        i = at[f"zwt=zisoi[{j}]"]
        assert (rows[hy.ZWT, i] == cols["zisoi"][i, s0 + j + 1]).all() and (rows[hy.ZWT, i] == cols["zisoi"][i, s0 + j + 1].astype(np.float32)).all()
    assert (rows[hy.HKSAT:hy.HKSAT + N, at["hksat=0"]] == 0.0).all()
    assert ((rows[hy.HKSAT:hy.HKSAT + N, at["hksat=0 in one layer"]] == 0.0).sum(axis=0) == 1).all()
    for name, v in (("frac_h2osfc=0", 0.0), ("frac_h2osfc=0.4", hy.PC), ("frac_h2osfc=1", 1.0)):
        assert (cols["frac_h2osfc"][at[name]] == v).all()
    for name, v in (("frac_sno_eff=0", 0.0), ("frac_sno_eff=1", 1.0)):
        assert (cols["frac_sno_eff"][at[name]] == v).all()
    i = at["ice beyond the pores"]
    over = cols["h2osoi_ice"][i, s0:s0 + N] / (cols["dz"][i, s0:s0 + N] * hy.DENICE) > cols["watsat"][i, :N]
    assert (over.sum(axis=1) >= 2).all()
    assert (cols["h2osoi_liq"][at["liq=0"], s0:s0 + N] == 0.0).all() and (cols["h2osoi_liq"][at["liq<1e-6"], s0:s0 + N] < 1.0e-6).all()
    i = at["root uptake beyond the water"]
    assert ((cols["qflx_rootsoi"][i, :N] * 1.0 > cols["h2osoi_liq"][i, s0:s0 + N]).sum(axis=1) >= 1).all()
    for name, key, v in (("bsw=1.5", "bsw", 1.5), ("bsw=20", "bsw", 20.0), ("sucsat=10", "sucsat", 10.0), ("sucsat=1000", "sucsat", 1000.0),
                         ("watsat=0.2", "watsat", 0.2), ("watsat=0.9", "watsat", 0.9)):
        assert (cols[key][at[name], :N] == v).all(), name
    i = at["t_soisno=tfrz at the front"]
    assert ((cols["t_soisno"][i, s0:s0 + N] == hy.TFRZ).sum(axis=1) >= 1).all()
    if frost:
        assert (fr[hy.Q_PERCH_MAX, at["q_perch_max=0"]] == 0.0).all()


def test_the_host_follows_ieee_and_poison_stays_in_its_column():
    """hydrology.step runs through the whole tier at every step length without raising; a poisoned column does not move its
    neighbours: every finite column gives the bits it gives when the columns of the non-finite tier are put back to the generator's
    values."""
    for frost in (False, True):
        g = edge_columns(257, SEED, frost=frost)
        poison = tuple(name for name in EDGE_CLASS_NAMES[EDGE_CLASS_NAMES.index("dz=0 in one layer"):])
        clean = edge_columns(257, SEED, frost=frost, skip=poison)
        fin = edge_finite(257)
        for dt in DTS:
            a = hy.step(g[0], g[1], dt, frost=g[2] if frost else None)
            b = hy.step(clean[0], clean[1], dt, frost=clean[2] if frost else None)
            for k in hy.WRITES:
                assert a[0][k][fin].tobytes() == b[0][k][fin].tobytes(), k
            assert a[1][:, fin].tobytes() == b[1][:, fin].tobytes()
            assert np.isfinite(b[1][:, fin]).all()
            if frost:
                assert a[2][:, fin].tobytes() == b[2][:, fin].tobytes()
