"""k_alb_tile - SNICAR of the one-layer snow packs and the final stage of albedo_snicar for a tile of 256 columns in one workgroup,
the products handed over in LDS - against the staged structure it replaces (ELMK_OPT_ALB_STAGED: k_alb_snicar<1> and k_alb_final as
launches of their own, meeting through the scratch array) and against the oracle.  Everything is compared bit for bit: every state
field, the error flags and the work-list counters.  Run on the GPU box: pytest -m gpu."""
import numpy as np
import pytest

from elmkernels_amd import state as st
from elmkernels_amd import synth
from tests import helpers as H

pytestmark = pytest.mark.gpu

DT = 1800.0
SN_MIN_SNW = 1.0e-30


def _one_layer(cols):
    """the columns k_alb_tile solves itself: sunlit, snow on the ground, one snow layer or none (the fictitious fresh-snow layer)"""
    return (cols["coszen"] > 0) & (cols["h2osno"] > SN_MIN_SNW) & (cols["snl"] <= 1)


def _deep(cols):
    return (cols["coszen"] > 0) & (cols["h2osno"] > SN_MIN_SNW) & (cols["snl"] >= 2)


def _same_everything(A, B, what):
    for k in list(A.fields) + ["err_flags"]:
        a, b = A[k], B[k]
        if a.dtype.kind == "f":
            same = bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())
        else:
            same = np.array_equal(a, b)
        assert same, (what, k)
    ca, cb = A.work_list_counters(), B.work_list_counters()
    # (the head of the canopy_fluxes queue is where the iteration kernel's waves stopped asking for more columns: it overshoots the
    #  queue's length by an amount that depends on their timing, with either structure, so it is no result)
    ca[0, 1] = cb[0, 1] = 0
    assert np.array_equal(ca, cb), (what, "work-list counters", ca.tolist(), cb.tolist())
    assert not ca[1].any() and not ca[2:8].any(), (what, "a work list was left non-empty", ca.tolist())


def _both_structures(cols, scal, soil, what):
    """the albedo wrapper through k_alb_tile (T) and through the staged structure (G) from identical uploads -> (T, G) as it left them"""
    T = H.device_state(cols, scal, soil)
    G = H.device_state(cols, scal, soil)
    G.set_option(st.OPT_ALB_STAGED, 1)
    st.kokkos_albedo_snicar(T)
    st.kokkos_albedo_snicar(G)
    _same_everything(T, G, f"{what}: albedo_snicar")
    return T, G


def _then_a_step(T, G, cols, what):
    """... and one full step on both, from the same upload again; closes them"""
    for D in (T, G):
        for k, v in cols.items():
            D[k] = v
        D.clear_errors()
        st.timestep7(D, DT)
    _same_everything(T, G, f"{what}: timestep7")
    T.close()
    G.close()


@pytest.mark.parametrize("tier,n,seed", [("B", 1, 201), ("B", 5, 202), ("B", 6, 203), ("B", 7, 204), ("B", 255, 205), ("B", 256, 206),
                                         ("B", 257, 207), ("B", 513, 208), ("A", 4700, 209)])
def test_tile_against_staged(tier, n, seed):
    """Every field after elmk_albedo_snicar and after one elmk_timestep7, option at 0 and at 1.  The branch-mix tier has night columns,
    bare ground and 0-5 snow layers, so a tile mixes columns whose products come from LDS and from the scratch array; the sizes
    put the end of the columns before, at and after the end of a six-column pass, of a wave and of a tile."""
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier=tier, seed=seed)
    if tier == "B" and n >= 255:
        assert _one_layer(cols).sum() > 20 and _deep(cols).sum() > 20 and (cols["coszen"] <= 0).sum() > 20
    if tier == "A":
        assert _one_layer(cols).sum() > 1000
    T, G = _both_structures(cols, scal, soil, f"{tier}/{n}")
    _then_a_step(T, G, cols, f"{tier}/{n}")


# ---- tiles built by hand from synth rows
_DONORS = {}


def _donors():
    """rows of one branch-mix state by kind, computed once: one resolved layer, the thin pack, five layers, snow-free"""
    if not _DONORS:
        ft = st.field_table()
        cols, scal, soil = synth.make_state(ft, 3008, tier="B", seed=77)
        snl, w = cols["snl"], cols["h2osno"]
        _DONORS.update(cols=cols, scal=scal, soil=soil, one=np.nonzero((snl == 1) & (w > 0))[0], thin=np.nonzero((snl == 0) & (w > 0))[0],
                       five=np.nonzero(snl == 5)[0], bare=np.nonzero((snl == 0) & (w == 0))[0], two=np.nonzero(snl == 2)[0])
        for k in ("one", "thin", "five", "bare", "two"):
            assert _DONORS[k].size >= 40, k
    return _DONORS


def _build(kinds):
    """kinds: one entry per column, 'one' / 'thin' / 'five' / 'two' / 'bare' (sunlit) or 'night' (a one-layer row without sun).
    Whole rows are taken, so snl, h2osno and the layers of a column agree; then coszen is set."""
    d = _donors()
    use = {k: 0 for k in ("one", "thin", "five", "bare", "two")}
    idx = np.empty(len(kinds), dtype=np.int64)
    for i, kind in enumerate(kinds):
        src = "one" if kind == "night" else kind
        idx[i] = d[src][use[src] % d[src].size]
        use[src] += 1
    cols = {k: np.ascontiguousarray(v[idx]) for k, v in d["cols"].items()}
    sun = np.array([0.9, 0.4, 0.1, 0.03])  # the last two: low sun, the zenith-angle correction of the near-infrared albedo
    cols["coszen"] = np.where(np.array([k == "night" for k in kinds]), -0.3, sun[np.arange(len(kinds)) % 4])
    # (the snow-free rows of the tile: nothing on the ground and no layer, whatever the donor row said)
    bare = np.array([k == "bare" for k in kinds])
    cols["snl"] = np.where(bare, 0, cols["snl"]).astype(np.int32)
    cols["h2osno"] = np.where(bare, 0.0, cols["h2osno"])
    return cols, d["scal"], d["soil"]


def _none(n):
    return [("five", "night", "bare", "two")[i % 4] for i in range(n)]


def _with_ones(n, where):
    kinds = _none(n)
    for j, i in enumerate(where):
        kinds[i] = "one" if j % 2 == 0 else "thin"
    return kinds


_HAND = {
    "every column of the tile": (["one" if i % 3 else "thin" for i in range(256)], 256),
    "none": (_none(256), 0),
    "exactly six": (_with_ones(256, (3, 64, 65, 130, 200, 255)), 6),
    "exactly seven": (_with_ones(256, (0, 63, 64, 127, 128, 191, 192)), 7),
    "only in the last, partial tile": (_with_ones(300, range(257, 300, 2)), 22),
    "one and five layers alternating": (["one" if i % 2 == 0 else "five" for i in range(256)], 128),
}


@pytest.mark.parametrize("case", list(_HAND))
def test_hand_built_tiles(case):
    """The lengths of a tile's LDS list at which its walk changes: the longest (256 columns, 43 six-column passes over four waves,
    every LDS slot in use), none, one full pass and one column more, a list only in the tile that the end of the columns cuts short,
    and a tile in which every other column reads the scratch array.  Both structures agree in every field, and the wrapper's outputs
    are the oracle's, bit for bit."""
    kinds, n_one = _HAND[case]
    cols, scal, soil = _build(kinds)
    assert int(_one_layer(cols).sum()) == n_one
    T, G = _both_structures(cols, scal, soil, case)
    S = H.oracle_state(cols, scal, soil)
    S.albedo_snicar()
    fatal = ((T["err_flags"] | S["err_flags"]) & 0x7FF) != 0
    assert np.array_equal(T["err_flags"] & 0x7FF, S["err_flags"] & 0x7FF), f"{case}: fatal flag sets differ"
    worst, bad = H.compare_states(T, S, skip_cols=fatal if fatal.any() else None, bitwise=True)
    assert not bad, f"{case}: tile kernel against the oracle, worst rel err {worst:.3e}: {bad}"
    _then_a_step(T, G, cols, case)


def test_structure_change_on_one_context():
    """ELMK_OPT_ALB_STAGED toggled between calls on a context whose step was captured as a graph before the toggle: every call is the
    same step as on a context that never left the staged structure, and the work lists are empty after each."""
    n = 5000
    ft = st.field_table()
    cols, scal, soil = synth.make_state(ft, n, tier="B", seed=83)
    A = H.device_state(cols, scal, soil)
    A.set_option(st.OPT_ALB_STAGED, 1)
    B = H.device_state(cols, scal, soil)
    B.set_graph(True)
    for staged in (0, 0, 1, 1, 0):  # (first call: capture; second: replay)
        B.set_option(st.OPT_ALB_STAGED, staged)
        st.timestep7(A, DT)
        st.timestep7(B, DT)
        _same_everything(A, B, f"graph on, staged = {staged}")
    B.set_graph(False)
    for staged in (1, 0):
        B.set_option(st.OPT_ALB_STAGED, staged)
        st.kokkos_albedo_snicar(A)
        st.kokkos_albedo_snicar(B)
        _same_everything(A, B, f"graph off, staged = {staged}")
    A.close()
    B.close()
