"""The inputs of the hillslope lateral flow's tests, host and device (include/elmk.h "hillslope lateral flow"): the shapes (one column to
the stream, a chain of five, stars of in-degree 1, 2, 4 and 8, and "wide": 1001 columns over four workgroups, a random forest of
hillslopes with columns on no hillslope in between and the designed hillslopes that keep every branch of L1 - L3 taken in every step),
the columns under them, the census of the branches, uniform loam slopes for the budget and the physical tests, and the counted bounds
of the two budgets."""
import numpy as np

from elmkernels_amd import hydrology as hy
from tests.hydrology_cases import column as loam
from tests.hydrology_cases import generated

DT = 1800.0
NSTEPS = 5
N = hy.N
S0, S1 = hy.NLEVSNO, hy.NLEVSNO + N
NAN, INF = float("nan"), float("inf")
SHAPES = ("one", "chain5", "star1", "star2", "star4", "star8", "wide")
# the branches of L1 - L3 as hydrology.py marks them: jwt == N with inflow; g > 0; g < 0 (the downhill T); both clamps; the stream
# clamp; the rising walk ending inside a layer and reaching the surface; the falling walk; a column on no hillslope
BRANCHES = ("lat_aquifer_inflow", "lat_g_pos", "lat_g_neg", "lat_clamp_lo", "lat_clamp_hi", "lat_stream_clamp", "lat_rise_in_layer",
            "lat_rise_surface", "lat_fall", "lat_off_hillslope")
K_ANISO = 50.0


def _geometry(n, rng):
    dist, width = rng.uniform(20.0, 200.0, n), rng.uniform(10.0, 100.0, n)
    return dist, width, rng.uniform(0.5, 2.0, n) * dist * width


def star(k, extra=0):
    """Column 0 at the stream with k uphill neighbours 1 .. k, each 3 m above it, and `extra` more columns in a chain above column 1."""
    n = 1 + k + extra
    down = np.zeros(n, np.int32)
    down[0] = -1
    for i in range(extra):
        down[1 + k + i] = 1 if i == 0 else k + i
    elev = np.concatenate([[1.0], 4.0 + 0.5 * np.arange(k), 8.0 + 2.0 * np.arange(extra)])
    return down, elev


def forest(n, rng):
    """(down, elev) of n columns: groups of 1 .. 12 consecutive columns, each a tree rooted at the stream whose columns lie up to 5 m
    above or 1 m below the column they drain into; one group in five is on no hillslope."""
    down = np.full(n, -2, np.int32)
    elev = np.zeros(n)
    c = 0
    while c < n:
        m = min(int(rng.integers(1, 13)), n - c)
        if rng.random() >= 0.2:
            deg = np.zeros(m, np.int64)
            down[c], elev[c] = -1, rng.uniform(-1.0, 3.0)
            for i in range(1, m):
                ok = np.nonzero(deg[:i] < hy.HS_MAXUP)[0]
                p = int(ok[rng.integers(0, ok.size)])
                deg[p] += 1
                down[c + i], elev[c + i] = c + p, elev[c + p] + rng.uniform(-1.0, 5.0)
        c += m
    return down, elev


# the designed hillslopes of the wide shape: (columns, down, elev, dist, width, area, ZWT or None) per hillslope; the columns are tamed
# (thawed, half saturated, no rain) unless the entry says otherwise
W_AQUIFER = (40, 41)      # 41 (ZWT 2 m) drains into 40 (ZWT 12 m: jwt == N, no transmissivity of its own), 40's head is below the stream
W_SURFACE = (50, 51)      # 51 (1 km2) drains into 50 (1 m2, ZWT 0.05 m) down a slope past the clamp: 50 fills to the surface every step
W_INLAYER = (60, 61)      # 61 drains into 60 (ZWT 2.5 m) gently: the rising walk ends in 60's water-table layer
W_UPHILL = (70, 71, 72)   # 72 lies below 71 (g < 0, the downhill T); 71 lies far below 70 (g < -2: the clamp)
W_BOUNDARY = (255, 256)   # 255 drains into 256 across the workgroup boundary
W_EDGE_ZWT = {80: NAN, 82: INF, 84: -INF, 86: 0.0, 88: 80.0}  # column c with this ZWT drains into column c + 1 at the stream
W_FROZEN = (90, 91)       # 90: every layer full of ice; drains into 91
W_DESIGNED = W_AQUIFER + W_SURFACE + W_INLAYER + W_UPHILL + W_BOUNDARY + W_FROZEN + tuple(c for k in W_EDGE_ZWT for c in (k, k + 1))


def shape(name, seed=3):
    """dict(ncols, down, dist, width, area, elev, k_aniso) of one shape."""
    rng = np.random.default_rng(seed)
    if name == "one":
        down, elev = np.array([-1], np.int32), np.array([2.0])
    elif name == "chain5":
        down, elev = np.array([-1, 0, 1, 2, 3], np.int32), np.array([1.0, 2.5, 4.0, 6.5, 9.0])
    elif name.startswith("star"):
        down, elev = star(int(name[4:]), extra=2)
    elif name == "run":  # the run, restart and tape tests': river_cases.run_case's 193 columns
        down, elev = forest(193, rng)
    elif name == "wide":
        n = 1001
        down, elev = forest(n, rng)
        d = lambda u, v: down.__setitem__(u, v)  # noqa: E731
        for u in W_DESIGNED:
            down[down == u] = -1  # whoever drained into a designed column drains into the stream
        d(40, -1), d(41, 40), d(50, -1), d(51, 50), d(60, -1), d(61, 60), d(70, -1), d(71, 70), d(72, 71), d(256, -1), d(255, 256)
        d(91, -1), d(90, 91)
        elev[[40, 41]] = -5.0, 3.0
        elev[[50, 51]] = -1.0, 400.0
        elev[[60, 61]] = 1.0, 3.0
        elev[[70, 71, 72]] = 500.0, 3.0, 2.0
        elev[[256, 255]] = 1.0, 4.0
        elev[[91, 90]] = 1.0, 4.0
        for k in W_EDGE_ZWT:
            d(k + 1, -1), d(k, k + 1)
            elev[[k + 1, k]] = 1.0, 4.0
    else:
        raise ValueError(name)
    n = down.size
    dist, width, area = _geometry(n, rng)
    if name == "wide":
        dist[list(W_DESIGNED)], width[list(W_DESIGNED)], area[list(W_DESIGNED)] = 100.0, 50.0, 5000.0
        area[[50, 51]] = 1.0, 1.0e6
        area[[40, 41]] = 500.0, 5000.0
        dist[41], width[41] = 1000.0, 1.0  # (a trickle: 40's water table stays below the column)
    return dict(name=name, ncols=n, down=down, dist=dist, width=width, area=area, elev=elev, k_aniso=K_ANISO)


def lat_of(G):
    """The `lat` of hydrology.step."""
    return G["down"], G["dist"], G["width"], G["area"], G["elev"], G["k_aniso"]


def tame(cols, rows, idx, zwt=2.0):
    """Columns idx thawed, snow-free, half saturated, without rain, uptake, surface water or evaporation, ZWT = zwt."""
    idx = np.atleast_1d(idx)
    dzmm = cols["dz"][idx, S0:S1].astype(np.float64) * 1.0e3
    cols["h2osoi_liq"][idx, S0:S1] = 0.5 * cols["watsat"][idx, :N] * dzmm
    cols["h2osoi_ice"][idx, S0:S1] = 0.0
    for k in ("qflx_top_soil", "h2osfc", "frac_h2osfc", "qflx_ev_h2osfc", "qflx_evap_grnd", "qflx_ev_soil", "qflx_dew_grnd", "qflx_dew_snow",
              "qflx_sub_snow"):
        cols[k][idx] = 0.0
    cols["qflx_rootsoi"][idx] = 0.0
    rows[hy.ZWT, idx] = zwt
    rows[hy.WA, idx] = 4000.0


def columns(G, seed):
    """(cols, scal, soil, rows) under a shape: the soil hydrology's generated tier (snow cleared in seven of eight columns); in the wide
    shape the designed columns are tamed and take their water tables, ice and edge values."""
    cols, scal, soil, rows = generated(G["ncols"], seed, full=True, chain=True)
    if G["name"] == "wide":
        tame(cols, rows, list(W_DESIGNED))
        rows[hy.ZWT, 40] = 12.0
        rows[hy.ZWT, 50] = 0.05
        rows[hy.ZWT, 60] = 2.5
        for k, v in W_EDGE_ZWT.items():
            rows[hy.ZWT, k] = v
        dzmm = cols["dz"][90, S0:S1].astype(np.float64) * 1.0e3
        cols["h2osoi_ice"][90, S0:S1] = cols["watsat"][90, :N] * dzmm * 0.917
        cols["h2osoi_liq"][90, S0:S1] = 0.02
    return cols, scal, soil, rows


STEP_FIELDS = hy.READS + ("h2osoi_vol",)


def host_chain(G, cols, rows, nsteps=NSTEPS, dt=DT, on=True, stored=None):
    """nsteps chained hydrology.step on the host from the generator's columns; returns per step (fields, rows, hs rows or None, hit)."""
    f = {k: np.array(cols[k]) for k in STEP_FIELDS}
    out = []
    for _ in range(nsteps):
        hit = set()
        res = hy.step(f, rows, dt, hit, stored=stored, lat=lat_of(G) if on else None)
        f = dict(f)
        f.update(res[0])
        rows = res[1]
        out.append((f, rows, res[2] if on else None, hit))
    return out


# ---- uniform loam slopes: the budget and the physical tests ----------------------------------------------------------------------------
def loam_fields(ncols, rain=0.0, evap=0.0, zwt=2.0, hksat=5.0e-3, sat=0.6):
    """ncols equal thawed, snow-free loam columns on ELM's grid (hydrology_cases.column) as the fields hydrology.step and
    water_balance_end read, under uniform rain that all reaches the soil, and their rows."""
    c = loam(sat=sat)
    lev = lambda a, tail=0.0: np.concatenate([np.zeros(hy.NLEVSNO), np.asarray(a, dtype=np.float64), np.full(20 - hy.NLEVSNO - len(a), tail)])  # noqa: E731
    f = {"h2osoi_liq": np.tile(lev(c["liq"]), (ncols, 1)), "h2osoi_ice": np.zeros((ncols, 20)), "dz": np.tile(lev(c["dz"], 1.0), (ncols, 1)),
         "zsoi": np.tile(lev(c["z"], 10.0), (ncols, 1)),
         "zisoi": np.tile(np.concatenate([np.zeros(hy.NLEVSNO), np.asarray(c["zi"]), np.full(21 - hy.NLEVSNO - N - 1, 10.0)]), (ncols, 1))}
    for k in ("watsat", "sucsat", "bsw"):
        f[k] = np.tile(np.concatenate([np.asarray(c[k]), np.full(15 - N, c[k][0])]), (ncols, 1))
    f["h2osoi_vol"], f["qflx_rootsoi"], f["snl"] = np.zeros((ncols, 15)), np.zeros((ncols, 15)), np.zeros(ncols, np.int32)
    for k in ("h2osfc", "frac_h2osfc", "frac_sno_eff", "qflx_ev_soil", "qflx_ev_h2osfc", "qflx_dew_grnd", "qflx_dew_snow", "qflx_sub_snow",
              "h2ocan", "h2osno", "qflx_snwcp_liq", "qflx_snwcp_ice", "forc_snow"):
        f[k] = np.zeros(ncols)
    f["qflx_evap_grnd"] = np.full(ncols, float(evap))
    f["qflx_evap_tot"] = f["qflx_evap_grnd"].copy()
    f["qflx_top_soil"] = np.full(ncols, float(rain))
    f["forc_rain"] = f["qflx_top_soil"].copy()
    rows = np.zeros((hy.NROWS, ncols))
    rows[hy.ZWT], rows[hy.WA] = zwt, 4000.0
    rows[hy.HKSAT:hy.HKSAT + N] = hksat
    rows[hy.WTFACT], rows[hy.H2OSFC_THRESH], rows[hy.K_WET], rows[hy.RSUB_TOP_MAX] = 0.3, 5.0, 0.05, 1.0e-4
    return f, rows


def slope5(flat=False):
    """Five columns in a chain, the toe (column 0) at the stream: 50 m apart, 30 m wide, 1500 m2 each, 3 m of fall per column (flat:
    every surface so that the heads are equal at ZWT 2 m and the toe's head is zero)."""
    down = np.array([-1, 0, 1, 2, 3], np.int32)
    elev = np.full(5, 2.0) if flat else 3.0 + 3.0 * np.arange(5)
    return dict(name="slope5", ncols=5, down=down, dist=np.full(5, 50.0), width=np.full(5, 30.0), area=np.full(5, 1500.0), elev=elev,
                k_aniso=K_ANISO)


U = 2.0 ** -53
# The per-column budget (hydrology.water_balance_end's ERRH2O) of the loam slope over six chained steps with the extension on.  The
# bound counts the statement's roundings of a column of at most W_MAX = 8192 mm of water (soil, surface and aquifer; the slope's columns
# hold under 6000): W1 adds 23 terms and W2 one more (24 roundings of at most u W_MAX each); W4 has 6 operations on values no larger;
# the stage moves water between the layers, the surface store and the aquifer in D.9, E, L3 / F.2, F.4 - F.7 and G, at most 8 updates of
# each of the 12 stores, each rounded to at most u times the store, and the stores sum to at most W_MAX (8 u W_MAX); ZWT is not part of
# the mass.  38 u W_MAX.  The measured value is the largest |ERRH2O| of the host test, extension on; off it measures the same order.
W_MAX = 8192.0
ERRH2O_BOUND = 38.0 * U * W_MAX
ERRH2O_MEASURED = 8.738565426824607e-13  # mm: the largest |ERRH2O| of the six-step host chain on the loam slope (step 1)


def l2_bound(G, hs):
    """Consequence 3's roundings, m3/s: per edge the owner's 1e3 vol / area (two roundings) and the receiver's (two more, and one per
    slot's addition), and the net's subtraction - at most 12 roundings per column, each of at most u times the larger flux of the
    column, as volume (area / 1e3)."""
    a = G["area"] * 1.0e-3
    return 1.01 * U * 12.0 * float((a * np.maximum(np.abs(hs[hy.HS_QLAT_OUT]), np.abs(hs[hy.HS_QLAT_IN]))).sum())


def hillslope_budget_bound(G, hs, dt=DT):
    """The bound of the hillslope's budget over one step, m3: the storage change of the columns, as volume, against dt (rain less
    evaporation less the surface runoff, less sum QSTREAM).  Every column brings its own ERRH2O, at most ERRH2O_BOUND, as volume;
    sum(area * QLAT_NET) * 1e-3 differs from sum(QSTREAM) by consequence 3's roundings (l2_bound) and by the two roundings per column
    of area * 1e-3 * QLAT_NET; both times dt."""
    a = G["area"] * 1.0e-3
    return float(a.sum()) * ERRH2O_BOUND + dt * (l2_bound(G, hs) + 2.0 * U * float(np.abs(a * hs[hy.HS_QLAT_NET]).sum()))


# The largest residual of that budget over the six chained steps of the loam slope (slope5), m3, in exact arithmetic on the host
# (step 3), and the bound hillslope_budget_bound gives for that step; sum QSTREAM dt is 0.49 m3 there.
HILLSLOPE_BUDGET_MEASURED = 2.450e-12
HILLSLOPE_BUDGET_BOUND = 2.592e-10
