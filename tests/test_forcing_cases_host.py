"""tests/forcing_cases.py on the host, without a GPU: reference(...) on the edge inputs takes both sides of every branch of the forcing
step, counted from its own outputs and intermediates, and every planted special is where its name says - the condition that keeps
tests/test_gpu_forcing_matrix.py from being vacuous.  Where oracle/_ref is built, reference(...) in REFERENCE mode is also pinned to
the reference's own get_forcing bit for bit on the same records."""
import numpy as np
import pytest

from elmkernels_amd import regrid as RG
from oracle import oracle as O
from tests import forcing_cases as FC
from tests.support import same, same_nan

TFRZ = FC.TFRZ
SIZES = (256, 257, 1001)
REC_DAY = 172.25  # the 06:00 record of the June solstice: day, night, dawn and dusk over the globe


def _both(mask, what):
    assert mask.any() and (~mask).any(), f"{what}: one side only ({int(mask.sum())} of {mask.size})"


@pytest.fixture(scope="module", params=SIZES)
def E(request):
    return FC.edge_records(request.param, 900 + request.param)


def test_planted_columns_are_distinct_and_hold_their_values(E):
    P = {k: v for k, v in E["planted"].items() if v is not None}
    assert len(set(P.values())) == len(P) >= 40
    rec, below, above = E["rec"], lambda v: np.nextafter(v, -np.inf), lambda v: np.nextafter(v, np.inf)
    for stream, tag, v in (("atm_tbot", "tbot_323", 323.0), ("atm_tbot", "tbot_tfrz", TFRZ), ("atm_tbot", "tbot_tfrz2", TFRZ + 2.0),
                           ("atm_pbot", "pbot_4e4", 4.0e4), ("atm_flds", "flds_50", 50.0), ("atm_flds", "flds_600", 600.0)):
        for side, want in (("below", below(v)), ("at", v), ("above", above(v))):
            assert (rec[stream][:, P[f"{tag}_{side}"]] == want).all(), (tag, side)
    assert (rec["atm_tbot"][:, P["tbot_cold"]] < TFRZ - 50.0).all() and (rec["atm_tbot"][:, P["tbot_hot"]] > TFRZ + 50.0).all()
    assert (rec["atm_qbot"][:, P["qbot_1e-9"]] == 1.0e-9).all() and (rec["atm_qbot"][:, P["qbot_below"]] < 1.0e-9).all()
    assert (rec["atm_qbot"][:, P["qbot_zero"]] == 0.0).all() and (rec["atm_qbot"][:, P["qbot_negative"]] < 0.0).all()
    assert (E["rh"][:, P["rh_0"]] == 0.0).all() and (E["rh"][:, P["rh_100"]] == 100.0).all()
    assert (rec["atm_prec"][:, P["prec_negative"]] < 0.0).all() and (rec["atm_fsds"][:, P["fsds_zero"]] == 0.0).all()
    z, nz = rec["atm_prec"][0, P["prec_zero"]], rec["atm_prec"][0, P["prec_negzero"]]
    assert z == 0.0 and not np.signbit(z) and nz == 0.0 and np.signbit(nz)
    dz = E["hc"] - E["hf"]
    assert dz[P["dz_zero"]] == 0.0 and dz[P["dz_plus3000"]] == 3000.0 and dz[P["dz_minus3000"]] == -3000.0
    assert (np.abs(dz) <= 3000.0).all() and (dz == 0.0).sum() >= E["n"] // 20 and (dz > 0).any() and (dz < 0).any()
    # groups: a column in none, the last column alone, and - past one workgroup - a group on both sides of column 256
    ptr, col, w = E["groups"]
    n = E["n"]
    assert P["no_group"] not in col.tolist() and np.setdiff1d(np.arange(n), col).tolist() == [P["no_group"]]
    assert ptr[-1] - ptr[-2] == 1 and col[-1] == P["one_column_group"]
    if n > 256:
        g = E["cell_of_col"]
        assert g[255] == g[256] >= 0


@pytest.mark.parametrize("rh", [False, True])
def test_reference_mode_takes_both_sides_of_every_branch(E, rh):
    P = E["planted"]
    R = FC.reference(FC.rec_for(E, rh), FC.edge_weights("exact"), rh, np.full(E["n"], 0.4))
    I = R["info"]
    # ProcessTBOT, PBOT, QBOT: the clamps, and the planted values through them
    _both(I["tbot_interp"] > 323.0, "tbot clamp")
    assert R["forc_tbot"][P["tbot_323_above"]] == 323.0 == R["forc_tbot"][P["tbot_323_at"]] == R["forc_tbot"][P["tbot_hot"]]
    assert R["forc_tbot"][P["tbot_323_below"]] == np.nextafter(323.0, 0.0) and same(R["forc_thbot"], R["forc_tbot"])
    _both(I["pbot_interp"] < 4.0e4, "pbot clamp")
    assert R["forc_pbot"][P["pbot_4e4_below"]] == 4.0e4 and R["forc_pbot"][P["pbot_4e4_above"]] == np.nextafter(4.0e4, 1e9)
    _both(I["qbot_interp"] < 1.0e-9, "qbot clamp")
    if rh:
        _both(R["forc_tbot"] > TFRZ, "esatw / esati")
        _both(R["forc_tbot"] - TFRZ < -50.0, "tdc's lower clamp")
        assert not (R["forc_tbot"] - TFRZ > 50.0).any()  # the upper one is behind the clamp at 323
        assert 0.0 < R["forc_qbot"][P["rh_0"]] < 1.0e-10 < R["forc_qbot"][P["rh_100"]]  # RH 0 is clamped at 1e-9 per cent
        t = [R["forc_qbot"][P[f"tbot_tfrz_{s}"]] / E["rh"][0, P[f"tbot_tfrz_{s}"]] for s in ("below", "at", "above")]
        assert np.isfinite(t).all()
    else:
        for name in ("qbot_1e-9", "qbot_below", "qbot_zero", "qbot_negative"):
            assert R["forc_qbot"][P[name]] == 1.0e-9, name
    # ProcessFLDS: <= 50 and >= 600 are computed, the doubles inside are taken as they are
    f = I["flds_interp"]
    assert (f <= 50.0).any() and (f >= 600.0).any() and ((f > 50.0) & (f < 600.0)).any()
    for name, computed in (("flds_50_below", True), ("flds_50_at", True), ("flds_50_above", False), ("flds_600_below", False),
                           ("flds_600_at", True), ("flds_600_above", True)):
        c = P[name]
        assert (R["forc_lwrad"][c] != f[c]) == computed, name
    # ProcessPREC: the record's clamp at 0 and the three ranges of frac2
    assert R["forc_rain"][P["prec_negative"]] == 0.0 == R["forc_snow"][P["prec_negative"]]
    for name in ("prec_zero", "prec_negzero"):
        assert R["forc_rain"][P[name]] == 0.0 and R["forc_snow"][P[name]] == 0.0, name
    wet = I["prec"] > 0.0
    frac1 = (R["forc_tbot"] - TFRZ) * 0.5
    assert (wet & (frac1 <= 0.0)).any() and (wet & (frac1 >= 1.0)).any() and (wet & (frac1 > 0.0) & (frac1 < 1.0)).any()
    assert R["forc_rain"][P["tbot_tfrz_at"]] == 0.0 and R["forc_rain"][P["tbot_tfrz_above"]] > 0.0
    assert R["forc_snow"][P["tbot_tfrz2_at"]] == 0.0 and R["forc_snow"][P["tbot_tfrz2_below"]] > 0.0
    # ProcessFSDS
    assert (R["forc_solad"][P["fsds_zero"]] == 0.0).all() and (R["forc_solad"] > 0.0).any()
    assert (R["forc_v"] == 0.0).all() and all((R[k] == 30.0).all() for k in ("forc_hgt",) + FC.HGT_PATCH)


def test_general_weights_read_both_records(E):
    wt = FC.edge_weights("general", 1)
    A = FC.reference(FC.rec_for(E, False), wt, False, np.full(E["n"], 0.4))
    rec2 = {k: v.copy() for k, v in E["rec"].items()}
    for k in rec2:
        rec2[k][1] += 1.0
    B = FC.reference(FC.rec_for(E, False, rec=rec2), wt, False, np.full(E["n"], 0.4))
    for k in ("forc_tbot", "forc_pbot", "forc_lwrad", "forc_u"):
        assert (A[k] != B[k]).any(), k
    for k in ("forc_solad", "forc_solai"):  # FSDS reads record t_idx only
        assert same(A[k], B[k]), k


def test_coszen_takes_both_sides_and_every_special(E):
    if not FC.have_cxx():
        pytest.skip("no g++")
    czf = FC.cosz_host(E["lat"], E["lon"], FC.FORC_DT, REC_DAY)
    _both(czf == 0.0, "czf == 0")
    cz, P = FC.edge_coszen(czf, 5)
    assert set(P) == {"cap_at", "cap_past", "cz_threshold", "cz_above_threshold", "czf_zero"} and len(set(P.values())) == 5
    R = FC.reference(FC.rec_for(E, False), FC.edge_weights("exact"), False, cz, czf=czf)
    fac = R["info"]["fac"]
    with np.errstate(all="ignore"):
        q = cz / czf
    _both(cz > 0.001, "cz > 0.001")
    _both((cz > 0.001) & (q > 10.0), "the cap")
    assert cz[P["cz_threshold"]] == 0.001 and fac[P["cz_threshold"]] == 0.0
    assert fac[P["cz_above_threshold"]] == np.nextafter(0.001, 1.0) / czf[P["cz_above_threshold"]] > 0.0
    assert q[P["cap_at"]] == 10.0 == fac[P["cap_at"]] and q[P["cap_past"]] > 10.0 and fac[P["cap_past"]] == 10.0
    assert czf[P["czf_zero"]] == 0.0 and cz[P["czf_zero"]] > 0.001 and fac[P["czf_zero"]] == 10.0
    assert np.isfinite(fac).all() and np.isfinite(R["forc_solad"]).all()
    off = FC.reference(FC.rec_for(E, False), FC.edge_weights("exact"), False, cz)
    assert not same(off["forc_solad"], R["forc_solad"]) and same(off["forc_tbot"], R["forc_tbot"])


@pytest.mark.parametrize("f32", [False, True])
def test_topo_takes_both_sides_and_every_special(E, f32):
    P = E["planted"]
    n = E["n"]
    args = (FC.rec_for(E, False), FC.edge_weights("exact"), False, np.full(n, 0.4))
    off = FC.reference(*args, f32=f32)
    R = FC.reference(*args, topo=FC.topo_of(E), f32=f32)
    I = R["info"]
    dz = I["dz"]
    assert (dz == 0.0).any() and (dz > 0.0).any() and (dz < 0.0).any()
    still = dz == 0.0
    for k in FC.FORC_FIELDS:
        assert same(R[k][still], off[k][still]), k
    assert (R["forc_tbot"][~still] != off["forc_tbot"][~still]).all()
    # the longwave band: the last double inside and the first outside, at both ends
    _both(I["hi"] < I["lin"], "upper end of the band")
    _both(I["lin"] < I["lo"], "lower end of the band")
    for name, outside, end in (("lw_upper_outside", True, "hi"), ("lw_upper_inside", False, "hi"), ("lw_lower_inside", False, "lo"),
                               ("lw_lower_outside", True, "lo")):
        c = P[name]
        assert I["lg"][c] == FC.BAND_LG, name
        assert (I["lc"][c] == I[end][c] and I["lin"][c] != I[end][c]) == outside, name
        assert (I["lc"][c] == I["lin"][c]) == (not outside), name
    c, d = P["lw_upper_outside"], P["lw_upper_inside"]
    assert np.nextafter(E["hc"][c], np.inf) == E["hc"][d]
    c, d = P["lw_lower_inside"], P["lw_lower_outside"]
    assert np.nextafter(E["hc"][c], np.inf) == E["hc"][d]
    # rain and snow split by the downscaled temperature where tbot alone would have split them otherwise
    tg, tc = I["tg"], I["tc"]
    c = P["tc_rain_to_snow"]
    assert tg[c] > TFRZ + 2.0 and tc[c] < TFRZ and R["forc_rain"][c] == 0.0 and off["forc_snow"][c] == 0.0 and R["forc_snow"][c] > 0.0
    c = P["tc_snow_to_rain"]
    assert tg[c] < TFRZ and tc[c] > TFRZ + 2.0 and R["forc_snow"][c] == 0.0 and off["forc_rain"][c] == 0.0 and R["forc_rain"][c] > 0.0
    for name in ("tc_snow_to_mixed", "tc_rain_to_mixed"):
        c = P[name]
        assert TFRZ < tc[c] < TFRZ + 2.0 and not TFRZ < tg[c] < TFRZ + 2.0 and R["forc_rain"][c] > 0.0 and R["forc_snow"][c] > 0.0, name
    # groups: columns of no group keep Lc, the one-column group gets back Lg (to rounding), every other group is rescaled
    G = FC.reference(*args, topo=FC.topo_of(E), groups=E["groups"], f32=f32)
    free = P["no_group"]
    assert G["forc_lwrad"][free] == R["forc_lwrad"][free]
    one = P["one_column_group"]
    tol = 4 * np.spacing(np.float32(off["forc_lwrad"][one])) if f32 else 4 * np.spacing(off["forc_lwrad"][one])
    assert abs(G["forc_lwrad"][one] - off["forc_lwrad"][one]) <= tol
    assert (G["info"]["norm"] != 1.0).any() and (G["forc_lwrad"] != R["forc_lwrad"]).any()
    for k in FC.FORC_FIELDS:
        if k != "forc_lwrad":
            assert same(G[k], R[k]), k
    if f32:
        for k in FC.FORC_FIELDS:
            assert same(G[k], FC.f32_round(G[k])), k


@pytest.mark.parametrize("width", range(1, 9))
def test_edge_map_holds_every_special_and_stays_finite(width):
    n, ncells = 257, 37
    idx, w, sp = FC.edge_map(width, n, ncells, 40 + width)
    assert idx.shape == w.shape == (width, n) and idx.dtype == np.int32 and (idx[0] >= 0).all() and idx.max() < ncells
    assert idx[0, 0] == 0 and idx[0, 1] == ncells - 1
    used = np.unique(idx[idx >= 0])
    assert sp["unused"].sum() == ncells - used.size >= 2 and sp["unused"][[5, ncells - 3]].all() and not sp["unused"][used].any()
    if width >= 2:
        assert idx[1, 2] == idx[0, 2]
        assert idx[1, 3] == sp["negzero"] and w[1, 3] == 0.0 and idx[width - 1, 4] == sp["huge"] and w[width - 1, 4] == 0.0
        assert (w[idx == sp["negzero"]] == 0.0).all() and (w[idx == sp["huge"]] == 0.0).all()
        assert (idx[1:] < 0).any()
    if width >= 3:
        assert idx[1, 5] == -1 and idx[2, 5] >= 0
    cells = FC.edge_cells(ncells, 50 + width, sp, nrec=2)
    h = FC.edge_heights(ncells, 60 + width, sp)
    for k in FC.STREAMS:
        a = cells[k]
        assert np.isnan(a[:, sp["unused"]]).all()
        if width >= 2:  # (a map of one row has no place for a term of weight 0: both cells are unreferenced there)
            assert (a[:, sp["huge"]] == FC.HUGE).all() and np.signbit(a[:, sp["negzero"]]).all()
        for f32 in (False, True):
            v = RG.apply_map(idx, w, FC.f32_round(a) if f32 else a)
            assert np.isfinite(v).all() and (np.abs(v) < 1.0e7).all(), (k, f32)
    assert np.isfinite(RG.apply_map(idx, w, h)).all()
    # through the whole step, every mode on: finite
    E = FC.edge_records(n, 70)
    R = FC.reference(cells, FC.edge_weights("general", 2), False, np.full(n, 0.3), grid=(idx, w), czf=np.full(n, 0.2),
                     topo=FC.topo_of(E, h), groups=E["groups"])
    for k in FC.FORC_FIELDS:
        assert np.isfinite(R[k]).all(), k
    assert same(R["info"]["hf"], RG.apply_map(idx, w, h))


def test_f32_rounds_inputs_first_and_outputs_last(E):
    args = (FC.rec_for(E, False), FC.edge_weights("general", 3), False, np.full(E["n"], 0.4))
    A = FC.reference(*args, f32=True)
    rounded = {k: FC.f32_round(v) for k, v in FC.rec_for(E, False).items()}
    B = FC.reference(rounded, *args[1:3], FC.f32_round(args[3]))
    for k in FC.FORC_FIELDS:
        assert same(A[k], FC.f32_round(B[k])), k
    assert not same(A["forc_tbot"], FC.reference(*args)["forc_tbot"])


def test_phenology_inputs_cover_every_rule():
    n = 1001
    Ph = FC.edge_phenology(n, 80)
    assert set(np.unique(Ph["vtype"]).tolist()) == {0, 1, 11, 12, 14}
    S = O.OracleState(n)
    for (m1, m2), wt1 in (((11, 0), 0.3), ((0, 1), 0.85)):
        for k, v in Ph["months"].items():
            S[k][:, 0], S[k][:, 1] = v[m1], v[m2]
        S["vtype"][:] = Ph["vtype"]
        S["snow_depth"][:] = Ph["snow_depth"]
        S["frac_sno"][:] = Ph["frac_sno"]
        S.phenology(wt1, 1.0 - wt1)
        veg = Ph["vtype"] != 0
        shrub = veg & (Ph["vtype"] <= 11)
        assert (S["tlai"][~veg] == 0.0).all() and (S["tlai"][veg] > 0.0).all()
        sd, hb, ht = Ph["snow_depth"], S["hbot"], S["htop"]
        assert (shrub & (sd < hb)).any() and (shrub & (sd > hb) & (sd < ht)).any() and (shrub & (sd > ht)).any()
        grass = veg & ~shrub
        assert (grass & (sd == 0.0)).any() and (grass & (sd == 0.2)).any() and (grass & (sd > 0.2)).any() and (grass & (sd == 0.1)).any()
        for k, t in (("elai", "tlai"), ("esai", "tsai")):
            small = veg & (S[t] < 0.1)
            assert (small & (S[k] == 0.0)).any() and (small & (S[k] >= 0.05)).any(), k
        _both(S["frac_veg_nosno_alb"] == 1, "frac_veg_nosno_alb")


@pytest.mark.parametrize("rh", [False, True])
def test_reference_mode_is_the_references_get_forcing(E, rh):
    """Where oracle/_ref is built: reference(...) in REFERENCE mode against elmref_get_forcing, bit for bit, on the edge records."""
    if not O.have_ref() or not hasattr(O.Reference().R, "elmref_get_forcing"):
        pytest.skip("oracle/_ref/libelmref.so not built (build() makes it where the reference is mounted)")
    n = E["n"]
    cz = np.random.default_rng(6).uniform(-0.2, 1.0, n)
    for kind in ("exact", "general"):
        wt = FC.edge_weights(kind, 4)
        rec = FC.rec_for(E, rh)
        got = FC.reference(rec, wt, rh, cz)
        S = O.OracleState(n)
        for k in FC.STREAMS:
            S[k][:, 0], S[k][:, 1] = rec[k][0], rec[k][1]
        S["coszen"][:] = cz
        S.get_forcing(wt[0], wt[1], rh, lib=O.Reference().R)
        for k in FC.FORC_FIELDS:
            assert same_nan(got[k], S[k]), (kind, k)
