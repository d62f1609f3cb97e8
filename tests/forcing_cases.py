"""The forcing step on the host, and the edge inputs the forcing tests share (tests/test_forcing_cases_host.py,
tests/test_gpu_forcing_matrix.py).

reference(...) is the one host statement of what a forcing kernel of k_forcing.hip writes, composed only of pieces that are pinned
on their own and none of which is device output: regrid.apply_map for the forcing grid, the oracle's get_forcing (pinned to the
reference's atm_physics_impl.hh bit for bit, tests/test_oracle_vs_ref.py) for the REFERENCE physics, shortwave.coszen_factor for
COSZEN, downscale.downscale_forcing with the oracle's qsat for TOPO, downscale.group_norm for the longwave groups.

edge_records / edge_map / edge_cells / edge_coszen / edge_phenology plant a value on every threshold those pieces branch on, in named
columns; the host test counts both sides of every branch from reference()'s own outputs and intermediates.

cosz_host is the host build of elmkernels_amd/csrc/elmk_solar.h (tests/c/solar_columns.cc, pinned to the reference's average_cosz by
tests/test_solar_geometry_host.py): the cos(zenith) of a step and of a forcing record's interval without a device.
"""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from elmkernels_amd import downscale as DSC
from elmkernels_amd import regrid as RG
from elmkernels_amd import state as st
from elmkernels_amd import synth
from elmkernels_amd.shortwave import coszen_factor
from oracle import oracle as O
from tests.support import ROOT

TFRZ = DSC.TFRZ
STREAMS = st.SERIES_FORCING  # atm_tbot, atm_pbot, atm_qbot, atm_flds, atm_fsds, atm_prec, atm_wind
# every (field, level) a forcing kernel writes; the last three are rewritten by init_timestep's kernel later in a step
FORC_ROWS = (("forc_tbot", 0), ("forc_thbot", 0), ("forc_pbot", 0), ("forc_qbot", 0), ("forc_lwrad", 0), ("forc_rain", 0),
             ("forc_snow", 0), ("forc_solad", 0), ("forc_solad", 1), ("forc_solai", 0), ("forc_solai", 1), ("forc_u", 0), ("forc_v", 0),
             ("forc_hgt", 0), ("forc_hgt_u_patch", 0), ("forc_hgt_t_patch", 0), ("forc_hgt_q_patch", 0))
HGT_PATCH = ("forc_hgt_u_patch", "forc_hgt_t_patch", "forc_hgt_q_patch")
FORC_FIELDS = tuple(dict.fromkeys(name for name, _ in FORC_ROWS))
# downscaling parameters of the tests: with them the longwave band of a 300 W/m2 column is reached at |dz| = 1800 m, inside +-3000 m
LAPSE, LAPSE_LW, LW_LIMIT = 0.0065, 0.05, 0.3
BAND_LG = 300.0  # the forcing longwave of the columns that sit on the band's edges (inside (50, 600): taken as it is)
FORC_DT = 3 * 3600.0  # the forcing records are 3-hourly means (COSZEN)
DT = 1800.0
HUGE = 3.0e38  # a huge cell value that fp32 still holds


def qsat(T, p):
    """(T, p) -> qs by the oracle's elmo_qsat."""
    return O.qsat(T, p)[2]


def f32_round(a):
    """The value a fp32 store leaves, widened again."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def reference(records, weights, rh, coszen, *, grid=None, czf=None, topo=None, groups=None, f32=False, stored_remap=False):
    """The forc_* rows one forcing step writes, on the host.

    records: {stream: [2, n]} - the two records that bracket the model time (level 0 and 1 of atm_*, or two slots of a series);
             cell records [2, ncells] with a grid.  weights: (wt1 [8], wt2 [8]).  rh: the QBOT stream is relative humidity in per cent.
    coszen:  [n], the step's cos(zenith).
    grid:    (idx, w) of the forcing map: every record goes through regrid.apply_map, and so do the forcing heights in TOPO mode.
    czf:     [n], the mean cos(zenith) of record 0's interval: COSZEN mode.  None: REFERENCE shortwave.
    topo:    (hc [n], hf, lapse, lapse_lw, lw_limit): TOPO mode; hf is [n], or [ncells] with a grid.
    groups:  (ptr, col, w): the longwave renormalisation groups (TOPO only).
    f32:     libelmk_f32.so - the kernels load fp32, compute in fp64 and store fp32: inputs are rounded to fp32 first (the records,
             and coszen, a state field), outputs last.  The elevations and czf stay fp64.  With groups, Lg is the unrounded fp64 value
             the forcing kernel hands k_ds_lw_norm, Lc the fp32 it reads back from forc_lwrad, and the product is rounded once more.
    stored_remap: the stepwise path - elmk_upload_gridded stores the remapped record in atm_* (at state precision) before the forcing
             kernel reads it, so with f32 the remap's result is rounded, not its cell values as in a run over cell series.

    Returns {field: [n] or [n, 2]} over FORC_FIELDS, and under "info" the intermediates the host test counts branches from."""
    wt1, wt2 = (np.ascontiguousarray(x, dtype=np.float64) for x in weights)
    r32 = f32_round if f32 else (lambda a: np.asarray(a, dtype=np.float64))
    rec = {k: np.asarray(records[k], dtype=np.float64)[:2] for k in STREAMS}
    with np.errstate(all="ignore"):
        if grid is None:
            cols = {k: r32(v) for k, v in rec.items()}
        elif stored_remap:
            cols = {k: r32(RG.apply_map(grid[0], grid[1], v)) for k, v in rec.items()}
        else:
            cols = {k: RG.apply_map(grid[0], grid[1], r32(v)) for k, v in rec.items()}
    n = cols[STREAMS[0]].shape[1]
    cz = r32(np.asarray(coszen, dtype=np.float64).reshape(-1))
    assert cz.shape == (n,)
    S = O.OracleState(n)
    for k in STREAMS:
        S[k][:, 0] = cols[k][0]
        S[k][:, 1] = cols[k][1]
    fac = None
    if czf is not None:
        czf = np.asarray(czf, dtype=np.float64).reshape(-1)
        fac = coszen_factor(cz, czf)
    S["coszen"][...] = (cz if fac is None else fac).reshape(S["coszen"].shape)
    S.get_forcing(wt1, wt2, rh)
    out = {k: S[k].copy() for k in FORC_FIELDS}
    with np.errstate(all="ignore"):
        info = {"tbot_interp": cols["atm_tbot"][0] * wt1[0] + cols["atm_tbot"][1] * wt2[0],
                "pbot_interp": cols["atm_pbot"][0] * wt1[1] + cols["atm_pbot"][1] * wt2[1],
                "qbot_interp": cols["atm_qbot"][0] * wt1[2] + cols["atm_qbot"][1] * wt2[2],
                "flds_interp": cols["atm_flds"][0] * wt1[3] + cols["atm_flds"][1] * wt2[3],
                "fsds": cols["atm_fsds"][0], "prec": cols["atm_prec"][0], "cz": cz, "czf": czf, "fac": fac,
                "tg": out["forc_tbot"].copy(), "lg": out["forc_lwrad"].copy()}
    if topo is not None:
        hc, hf, lapse, lapse_lw, lw_limit = topo
        hc = np.asarray(hc, dtype=np.float64).reshape(-1)
        hf = np.asarray(hf, dtype=np.float64).reshape(-1)
        if grid is not None:
            hf = RG.apply_map(grid[0], grid[1], hf)
        lg = out["forc_lwrad"]
        ds = DSC.downscale_forcing(out, cols["atm_prec"][0], hc, hf, qsat, lapse, lapse_lw, lw_limit)
        lc = ds["forc_lwrad"]
        with np.errstate(all="ignore"):
            dz = hc - hf
            info.update(hf=hf, dz=dz, lin=lg - lapse_lw * dz, hi=lg * (1.0 + lw_limit), lo=lg * (1.0 - lw_limit), tc=ds["forc_tbot"],
                        lc=lc.copy())
            if groups is not None:
                ptr, col, w = DSC.check_groups(*groups, n)
                lc = r32(lc)  # what k_ds_lw_norm reads back from forc_lwrad
                norm = DSC.group_norm(lg, lc, ptr, col, w)
                lc = lc.copy()
                lc[col] = lc[col] * np.repeat(norm, np.diff(ptr))
                info["norm"] = norm
        ds["forc_lwrad"] = lc
        out.update(ds)
    elif groups is not None:
        raise ValueError("groups without topo")
    out = {k: r32(v) for k, v in out.items()}
    out["info"] = info
    return out


# ---- cos(zenith) on the host ---------------------------------------------------------------------------------------------------------
_SOLAR = None


def have_cxx():
    return shutil.which("g++") is not None


def cosz_host(lat, lon, dt, decday):
    """average_cosz over dt seconds from decday (decimal_doy + 1.0) at every (lat, lon) in radians: the host build of elmk_solar.h, the
    routine k_solar.hip runs.  A step's coszen is cosz_host(lat, lon, dt, step decday); a record's czf is cosz_host(lat, lon, forc_dt,
    record decday)."""
    global _SOLAR
    if _SOLAR is None:
        d = tempfile.mkdtemp(prefix="elmk_solar_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "columns.so")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                               os.path.join(ROOT, "elmkernels_amd", "csrc"), os.path.join(ROOT, "tests", "c", "solar_columns.cc"), "-o", so])
        lib = C.CDLL(so)
        lib.elmk_test_solar_columns.argtypes = [C.c_long] + [C.c_void_p] * 9
        lib.elmk_test_solar_columns.restype = None
        _SOLAR = lib
    lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
    lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
    n = lat.size
    dts, days = np.full(n, float(dt)), np.full(n, float(decday))
    doy = np.full(n, int(decday) - 1, np.int32)
    out = [np.zeros(n) for _ in range(4)]
    _SOLAR.elmk_test_solar_columns(n, lat.ctypes.data, lon.ctypes.data, dts.ctypes.data, days.ctypes.data, doy.ctypes.data,
                                   *[o.ctypes.data for o in out])
    return out[0]


# ---- edge inputs ---------------------------------------------------------------------------------------------------------------------
def _nbr(v):
    """(the double below, v, the double above)"""
    return float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))


def _edge_pair(cond, x0):
    """Adjacent doubles (a, b), a < b, with cond(a) != cond(b), found by walking from x0 (which lies within a few ulps of the edge)."""
    for up in (np.inf, -np.inf):
        x, c0 = float(x0), cond(x0)
        for _ in range(4096):
            y = float(np.nextafter(x, up))
            if cond(y) != c0:
                return (x, y) if up > 0 else (y, x)
            x = y
    raise AssertionError("no edge near x0")


class _Columns:
    """Hands out distinct columns (while n allows: stride 7 from column 3, wrapping), and remembers each under its name."""

    def __init__(self, n):
        self.n, self.i, self.named = n, 0, {}

    def take(self, name):
        c = (3 + 7 * self.i) % self.n
        self.i += 1
        self.named[name] = c
        return c


def edge_weights(kind, seed=0):
    """(wt1, wt2): "exact" is (1, 0) for every stream, under which a planted value survives forc1 * wt1 + forc2 * wt2 exactly;
    "general" reads both records of every stream."""
    if kind == "exact":
        return np.ones(8), np.zeros(8)
    wt2 = 0.05 + 0.9 * np.random.default_rng(1000 + seed).random(8)
    return 1.0 - wt2, wt2


def edge_records(n, seed, nrec=2):
    """The per-column edge inputs of n columns -> a dict:
      rec      {stream: [nrec, n]}: random values in the ranges of run_cases._inputs with the specials below planted, the same value in
               every record of a planted column (so a special is level 0 of every step of a run);
      rh       [nrec, n]: the QBOT stream as relative humidity in per cent (rec_for(E, True) puts it in atm_qbot's place);
      hc, hf   [n] elevations; lat, lon [n] in radians over the globe; groups (ptr, col, w) of the longwave renormalisation;
      planted  {name: column} of every special (distinct columns while n >= 80; at smaller n later names win a shared column).
    Specials: tbot 323, TFRZ, TFRZ + 2 and the doubles beside each (ProcessTBOT's clamp, esatw / esati, frac2's clamps), TFRZ - 60
    (tdc's lower clamp; its upper one is out of reach behind the clamp at 323, which 330 takes); pbot 4e4 and neighbours; qbot 1e-9,
    5e-10, 0 and -1e-3; RH 0 and 100; flds 50, 600 and neighbours (<= and >= against the literals); prec -1e-4, 0.0, -0.0; fsds 0.0.
    TOPO: hc == hf; dz = +-3000 exactly; four columns whose lg - lapse_lw * dz is the last double inside and the first outside each
    end of the lw_limit band (flds = BAND_LG, hf = 0, under LAPSE_LW and LW_LIMIT); three columns whose downscaled temperature
    crosses TFRZ or TFRZ + 2 while tbot does not, and one that lands between them.
    Groups: about 50 columns each in column order (one spans columns 255 and 256 when n > 256), column 8 in no group, column 9 a
    group of its own (the last one of the map)."""
    ft = st.field_table()
    cols, _, _ = synth.make_state(ft, n, tier="B", seed=seed)
    rng = np.random.default_rng(seed + 2)
    rec = {}
    for k in STREAMS:
        a, b = cols[k][:, 0], cols[k][:, 1]
        t = np.linspace(0.0, 1.0, nrec)[:, None]
        rec[k] = (1.0 - t) * a[None, :] + t * b[None, :] + 0.01 * np.abs(a)[None, :] * rng.standard_normal((nrec, n))
    m = rng.random((nrec, n))
    rec["atm_flds"] = np.where(m < 0.05, 30.0, np.where(m > 0.95, 700.0, rec["atm_flds"]))
    rec["atm_prec"] = np.abs(rec["atm_prec"]) + 1.0e-5
    rec["atm_fsds"] = np.abs(rec["atm_fsds"]) + 1.0
    rh = np.clip(100.0 * rng.random((nrec, n)), 1.0, 99.0)
    hf = 200.0 + 1500.0 * rng.random(n)
    hc = hf + rng.uniform(-3000.0, 3000.0, n)
    hc[::10] = hf[::10]  # equal elevations on every tenth column (where a TOPO special below does not take the column)
    lat, lon = synth.global_grid(n, seed=seed + 1)
    P = _Columns(n)

    def plant(stream, name, v):
        c = P.take(name)
        (rh if stream == "rh" else rec[stream])[:, c] = v
        return c

    for base, tag in ((323.0, "tbot_323"), (TFRZ, "tbot_tfrz"), (TFRZ + 2.0, "tbot_tfrz2")):
        for v, side in zip(_nbr(base), ("below", "at", "above")):
            plant("atm_tbot", f"{tag}_{side}", v)
    plant("atm_tbot", "tbot_cold", TFRZ - 60.0)
    plant("atm_tbot", "tbot_hot", 330.0)
    for v, side in zip(_nbr(4.0e4), ("below", "at", "above")):
        plant("atm_pbot", f"pbot_4e4_{side}", v)
    for v, name in ((1.0e-9, "qbot_1e-9"), (5.0e-10, "qbot_below"), (0.0, "qbot_zero"), (-1.0e-3, "qbot_negative")):
        c = plant("atm_qbot", name, v)
        rh[:, c] = 50.0
    plant("rh", "rh_0", 0.0)
    plant("rh", "rh_100", 100.0)
    for base, tag in ((50.0, "flds_50"), (600.0, "flds_600")):
        for v, side in zip(_nbr(base), ("below", "at", "above")):
            plant("atm_flds", f"{tag}_{side}", v)
    for v, name in ((-1.0e-4, "prec_negative"), (0.0, "prec_zero"), (-0.0, "prec_negzero")):
        plant("atm_prec", name, v)
    plant("atm_fsds", "fsds_zero", 0.0)
    # TOPO
    for name, dz in (("dz_zero", 0.0), ("dz_plus3000", 3000.0), ("dz_minus3000", -3000.0)):
        c = P.take(name)
        hf[c] = 1000.0 if dz else hf[c]
        hc[c] = hf[c] + dz
    lg = BAND_LG
    hi, lo = lg * (1.0 + LW_LIMIT), lg * (1.0 - LW_LIMIT)
    up = _edge_pair(lambda d: hi < lg - LAPSE_LW * d, -lg * LW_LIMIT / LAPSE_LW)  # (dmin takes the band's end where hi < lin)
    dn = _edge_pair(lambda d: lg - LAPSE_LW * d < lo, lg * LW_LIMIT / LAPSE_LW)
    for name, dz in (("lw_upper_outside", up[0]), ("lw_upper_inside", up[1]), ("lw_lower_inside", dn[0]), ("lw_lower_outside", dn[1])):
        c = P.take(name)
        rec["atm_flds"][:, c] = lg
        rec["atm_tbot"][:, c] = 280.0
        hf[c], hc[c] = 0.0, dz
    for name, tb, dz in (("tc_rain_to_snow", TFRZ + 5.0, 1000.0), ("tc_snow_to_rain", TFRZ - 3.0, -1000.0),
                         ("tc_snow_to_mixed", TFRZ - 2.0, -500.0), ("tc_rain_to_mixed", TFRZ + 4.0, 400.0)):
        c = P.take(name)
        rec["atm_tbot"][:, c] = tb
        rec["atm_prec"][:, c] = 2.0e-4
        hf[c] = 500.0
        hc[c] = hf[c] + dz
    # groups
    cell = np.arange(n) // 50
    if n > 2:
        cell[min(8, n - 2)] = -1
    P.named["no_group"] = min(8, n - 2) if n > 2 else None
    one = 9 if n > 10 else n - 1
    if n > 1:
        cell[one] = cell.max() + 1
    P.named["one_column_group"] = one
    area = 0.5 + np.random.default_rng(seed + 3).random(n)
    groups = RG.owner_map(cell, area, int(cell.max()) + 1)
    return {"n": n, "rec": rec, "rh": rh, "hc": hc, "hf": hf, "lat": lat, "lon": lon, "groups": groups, "cell_of_col": cell,
            "planted": dict(P.named)}


def rec_for(E, rh, slot=0, rec=None):
    """{stream: [2, n]}: records slot and slot + 1 of E["rec"] (or of `rec`), the RH stream in atm_qbot's place when rh."""
    R = dict(E["rec"] if rec is None else rec)
    if rh:
        R["atm_qbot"] = E["rh"]
    return {k: R[k][slot:slot + 2] for k in STREAMS}


def topo_of(E, hf=None):
    return (E["hc"], E["hf"] if hf is None else hf, LAPSE, LAPSE_LW, LW_LIMIT)


def edge_coszen(czf, seed):
    """A step's cos(zenith) per column, given the record's czf -> (cz [n], planted {name: column}): random in [-0.2, 1], a third of
    the columns at or below 0.001, with cz == 0.001 and the double above it; cz / czf == 10.0 exactly and the first cz whose quotient is
    past 10 (on columns with czf > 0); cz = 0.5 on a column with czf == 0 (the cap must give 10, not inf or NaN).  A special that needs
    a kind of column czf does not have is left out of `planted`."""
    czf = np.asarray(czf, dtype=np.float64)
    n = czf.size
    rng = np.random.default_rng(seed)
    cz = np.where(rng.random(n) < 0.33, rng.uniform(-0.2, 0.001, n), rng.uniform(0.001, 1.0, n))
    planted = {}
    day = [c for c in np.nonzero(czf > 0.0)[0].tolist()]
    night = np.nonzero(czf == 0.0)[0].tolist()
    # cz / czf == 10 exactly: the columns whose 10 * czf divides back to 10.0 (most do)
    exact = [c for c in day if (10.0 * czf[c]) / czf[c] == 10.0 and 10.0 * czf[c] > 0.001 and 10.0 * czf[c] < 1.0]
    if len(exact) >= 2:
        a, b = exact[0], exact[1]
        cz[a] = 10.0 * czf[a]
        lo, hi = _edge_pair(lambda x: 10.0 < x / czf[b], 10.0 * czf[b])
        cz[b] = hi
        planted.update(cap_at=a, cap_past=b)
    free = [c for c in day if c not in planted.values()]
    if len(free) >= 2:
        cz[free[0]], cz[free[1]] = 0.001, np.nextafter(0.001, 1.0)
        planted.update(cz_threshold=free[0], cz_above_threshold=free[1])
    if night:
        cz[night[0]] = 0.5
        planted["czf_zero"] = night[0]
    return cz, planted


def edge_map(width, n, ncells, seed):
    """An ELL forcing map of `width` rows (1 .. 8; the host pads 3, 5, 6 and 7 to 4 or 8) over ncells >= 8 cells ->
    (idx int32 [width, n], w [width, n], cells) with cells = {"negzero": cell, "huge": cell, "unused": bool [ncells]}.
    Random cells and positive weights that sum to one per column, about a quarter of the rows behind row 0 padding (idx -1, w 0), and:
    column 0 starts at cell 0 and column 1 at cell ncells - 1; (width >= 2) column 2 repeats one cell in rows 0 and 1, column 3 carries
    weight 0.0 on the cell that holds -0.0 and column 4 weight 0.0 on the cell that holds HUGE (edge_cells puts them there; no other
    term points at either); (width >= 3) column 5 has idx -1 in row 1 and a valid row 2 behind it.  Cells 5 and ncells - 3 are
    referenced by no column, and `unused` marks every cell no column references: edge_cells sets them NaN."""
    assert 1 <= width <= RG.MAX_NPTS and ncells >= 8
    rng = np.random.default_rng(seed)
    negzero, huge = 2, ncells - 2
    ok = np.setdiff1d(np.arange(ncells), [negzero, huge, 5, ncells - 3])
    idx = ok[rng.integers(0, ok.size, (width, n))].astype(np.int32)
    w = 0.1 + rng.random((width, n))
    pad = rng.random((width, n)) < 0.25
    pad[0] = False
    special = min(n, 6)
    pad[:, :special] = False
    idx[pad] = -1
    w[pad] = 0.0
    w = w / w.sum(axis=0)

    def col(c):
        return c if c < n else None

    if col(0) is not None:
        idx[0, 0] = 0
    if col(1) is not None:
        idx[0, 1] = ncells - 1
    if width >= 2:
        if col(2) is not None:
            idx[1, 2] = idx[0, 2]
        if col(3) is not None:
            idx[1, 3], w[1, 3] = negzero, 0.0
        if col(4) is not None:
            idx[width - 1, 4], w[width - 1, 4] = huge, 0.0
    if width >= 3 and col(5) is not None:
        idx[1, 5], w[1, 5] = -1, 0.0
    unused = np.ones(ncells, bool)
    unused[idx[idx >= 0]] = False
    return idx, w, {"negzero": negzero, "huge": huge, "unused": unused}


def edge_cells(ncells, seed, special, nrec=2):
    """Cell records {stream: [nrec, ncells]} for edge_map's `special`: edge_records' values (its planted columns become cells), -0.0
    in the negzero cell and HUGE in the huge cell of every stream, NaN in every cell no column references."""
    rec = {k: v.copy() for k, v in edge_records(ncells, seed, nrec)["rec"].items()}
    for k in STREAMS:
        rec[k][:, special["negzero"]] = -0.0
        rec[k][:, special["huge"]] = HUGE
        rec[k][:, special["unused"]] = np.nan
    return rec


def edge_heights(ncells, seed, special):
    """Forcing surface heights per cell for edge_map's `special`: 200 .. 1700 m, -0.0 and HUGE where edge_cells has them, and -9e30 in
    every cell no column references (elmk_set_forcing_elevation_gridded refuses a non-finite height; this one poisons what reads it)."""
    h = 200.0 + 1500.0 * np.random.default_rng(seed).random(ncells)
    h[special["negzero"]] = -0.0
    h[special["huge"]] = HUGE
    h[special["unused"]] = -9.0e30
    return h


def edge_phenology(n, seed):
    """Phenology edge inputs -> {"vtype": int32 [n], "snow_depth", "frac_sno": [n], "months": {field: [12, n]}}: vtype over 0 (bare),
    1, 11 (the last shrub rule), 12 and 14 (the 0.2 m burial rule); canopy bottoms below tops; snow_depth at 0, below hbot, between
    hbot and htop, above htop, and at 0.1, 0.2 and 0.3 m; leaf and stem areas from 0.02 to 0.08 on every fourth column (elai and esai on
    either side of 0.05) and of order one elsewhere."""
    rng = np.random.default_rng(seed)
    vtype = rng.choice(np.array([0, 1, 11, 12, 14], np.int32), n).astype(np.int32)
    hbot = 0.05 + 2.0 * rng.random((12, n))
    htop = hbot + 0.05 + 5.0 * rng.random((12, n))
    lai = np.where(np.arange(n) % 4 == 0, rng.uniform(0.02, 0.08, (12, n)), rng.uniform(0.2, 6.0, (12, n)))
    sai = np.where(np.arange(n) % 4 == 1, rng.uniform(0.02, 0.08, (12, n)), rng.uniform(0.1, 2.0, (12, n)))
    kind = np.arange(n) % 7
    lo, hi = hbot.min(axis=0), htop.max(axis=0)
    snow = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                     [0.0, 0.5 * lo, 0.5 * (hbot.max(axis=0) + htop.min(axis=0)), hi + 1.0, 0.1, 0.2], 0.3)
    frac_sno = np.where(np.arange(n) % 5 == 0, 0.0, rng.random(n))
    return {"vtype": vtype, "snow_depth": snow, "frac_sno": frac_sno,
            "months": {"mlai": lai, "msai": sai, "mhtop": htop, "mhbot": hbot}}
