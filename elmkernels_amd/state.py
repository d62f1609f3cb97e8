"""ELMState: the host-side mirror of the reference's ELM::ELMState (src/data/elm_state.h:182-225) on top of
the libelmk context, and the seven physics entry points with the reference's wrapper names.

    S = ELMState(ncols, device=0)
    S["t_soisno"] = arr            # [ncols, 20], reference layout ([column][level])
    S.set_land(ltype=1, ctype=1, vtype=12)
    kokkos_canopy_hydrology(S, dt) # == ELM::kokkos_canopy_hydrology(S, dt) of driver/kokkos
    out = S["h2osno"]              # download

Everything numerical happens in HIP kernels behind the C ABI; this module only moves arrays and arguments.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from .downscale import DS_MODES, LAPSE, LAPSE_LW, LW_LIMIT
from .shortwave import SW_COSZEN, SW_MODES, SW_REFERENCE  # noqa: F401

DTYPES = {0: np.float64, 1: np.int32, 2: np.uint8, 3: np.uint32}
LAYOUT_COL_MAJOR, LAYOUT_SOA = 0, 1
OPT_CF_HALF_WORKGROUPS = 1  # elmk_set_option
OPT_ALB_STAGED = 2  # elmk_set_option: albedo_snicar as three stages instead of k_alb_tile
OPT_RESTART_CELLS = 3  # elmk_set_option: the restart image carries the routing state (version 6; restart.VERSION_ROUTING)
HIST_AVG, HIST_SUM, HIST_MAX, HIST_MIN, HIST_INST = range(5)  # elmk_history_add
HIST_OPS = {"avg": HIST_AVG, "sum": HIST_SUM, "max": HIST_MAX, "min": HIST_MIN, "inst": HIST_INST}
HIST_MAX_TAPES, HIST_MAX_ENTRIES = 4, 64
CLASS_PROGNOSTIC, CLASS_SURFACE, CLASS_FORCING, CLASS_DIAGNOSTIC = range(4)  # elmk_field_class
CLASS_NAMES = ("prognostic", "surface", "forcing", "diagnostic")
RUN_QBOT_IS_RH, RUN_HISTORY, RUN_ACCUM, RUN_AEROSOL, RUN_ALT, RUN_HYDROLOGY = 1, 2, 4, 8, 16, 32  # elmk_run flags
RUN_WATER_BALANCE = 64  # every step closes the water budget (water_balance_enable; needs RUN_HYDROLOGY)
RUN_IRRIGATION = 128  # every step applies and checks irrigation between the seven wrappers and soil_temperature (irrigation_enable)
IRR_RATE, IRR_NLEFT, IRR_QFLX_IRRIG = range(3)  # elmk_irrigation_read (irrigation.RATE .. irrigation.QFLX_IRRIG)
IRR_NROWS = 3
IRRSUP_DEMAND, IRRSUP_COMMITTED, IRRSUP_RATIO, IRRSUP_UNMET_SUM = range(4)  # elmk_irrigation_supply_read (irrigation.DEMAND .. UNMET_SUM)
IRRSUP_NROWS = 4
RUN_ROUTING = 256  # every step routes the step's runoff after the water balance (routing_enable; needs RUN_WATER_BALANCE)
ROUTE_VOLR, ROUTE_QIN, ROUTE_QOUT, ROUTE_QOUT_SUM = range(4)  # elmk_routing_read (routing.VOLR .. routing.QOUT_SUM)
ROUTE_WH, ROUTE_WT, ROUTE_QSUR = 4, 5, 6  # ... while the kinematic-wave scheme is on (routing.WH, routing.WT, routing.QSUR)
ROUTE_KW_NPARAM = 11  # the rows of routing_kinematic_enable's params (routing.HSLP .. routing.NR)
ROUTE_WF, ROUTE_FLOOD_DEPTH, ROUTE_FLOOD_FRAC = 7, 8, 9  # ... while the floodplain inundation is on (routing.WF .. routing.FLOOD_FRAC)
ROUTE_FP_NPROF = 11  # the rows of routing_inundation_enable's eprof
ROUTE_RES, ROUTE_KRLS, ROUTE_RES_TAKE = 10, 11, 12  # ... while the reservoirs are on (routing.RES .. routing.RES_TAKE)
ROUTE_TT, ROUTE_TR, ROUTE_HEAT, ROUTE_HIN, ROUTE_HSRF, ROUTE_HADJ, ROUTE_HOUT = range(13, 20)  # ... while the stream temperature is on (routing.TT .. routing.HOUT)
WB_NROWS = 7  # elmk_water_balance_read: the row numbers are hydrology.WB_BEGWB .. hydrology.WB_TOTSOILICE
ROWS_ALT, ROWS_HYDROLOGY, ROWS_FROST, ROWS_WATER_BALANCE, ROWS_IRRIGATION = range(5)  # history_add_row: the feature families (ELMK_ROWS_*)
ROWS_FLOODPLAIN = 7  # ... and the floodplain infiltration's (ELMK_ROWS_FLOODPLAIN; which = FPI_*), past the cell-row families' numbers
FPI_H2OROF, FPI_FRAC, FPI_QFLX_DRAIN = range(3)  # floodplain_infiltration_read (hydrology.FPI_*)
ROWS_HILLSLOPE = 8  # ... and the hillslope lateral flow's (ELMK_ROWS_HILLSLOPE; which = HS_*)
HS_HEAD, HS_TRANS, HS_QLAT_OUT, HS_QLAT_IN, HS_QLAT_NET, HS_QSTREAM = range(6)  # hillslope_read (hydrology.HS_*)
HS_NROWS = 6
ROUTE_QLAND = 20  # routing_read while the floodplain infiltration is on (routing.QLAND)
ROUTE_CMD_WANT, ROUTE_CMD_TAKE, ROUTE_CMD_GIVE, ROUTE_CMD_RATIO = 21, 22, 23, 24  # ... while the command areas are on (routing.CMD_WANT ..)
ROUTE_CMD_NDEP = 4  # ELMK_CMD_NDEP: the slots of a cell's dependency rows
ROW_FAMILIES = {"alt": ROWS_ALT, "hydrology": ROWS_HYDROLOGY, "frost": ROWS_FROST, "water_balance": ROWS_WATER_BALANCE,
                "irrigation": ROWS_IRRIGATION, "floodplain": ROWS_FLOODPLAIN, "hillslope": ROWS_HILLSLOPE}
CELL_ROWS_ROUTING, CELL_ROWS_SUPPLY = range(2)  # cell_history_add_row: the cell-row families (ELMK_CELL_ROWS_*)
CELL_ROW_FAMILIES = {"routing": CELL_ROWS_ROUTING, "supply": CELL_ROWS_SUPPLY}
HYD_NROWS, HYD_NLAYER = 23, 10 # elmk_soil_hydrology_read: the row numbers are hydrology.ZWT .. hydrology.FSAT
HYDF_NROWS = 4  # elmk_soil_hydrology_frost_read: hydrology.Q_PERCH_MAX .. hydrology.QFLX_DRAIN_PERCHED
ALT_ALT, ALT_ALTMAX, ALT_ALTMAX_LASTYEAR = range(3)  # elmk_active_layer_read
ALT_ROLL_NORTH, ALT_ROLL_SOUTH = 1, 2  # elmk_active_layer_update
ACCUM_RUNMEAN, ACCUM_TIMEAVG, ACCUM_RUNACCUM = range(3)  # elmk_accum_add
ACCUM_KINDS = {"runmean": ACCUM_RUNMEAN, "timeavg": ACCUM_TIMEAVG, "runaccum": ACCUM_RUNACCUM}
ACCUM_MAX_ENTRIES = 16
# elmk_run_step of include/elmk.h, field for field (natural C alignment: tests/test_run_host.py checks it against gcc)
RUN_STEP_DTYPE = np.dtype([("decday", np.float64), ("doy", np.int32), ("forc_slot", np.int32), ("forc_wt1", np.float64, (8,)),
                           ("forc_wt2", np.float64, (8,)), ("month1", np.int32), ("month2", np.int32), ("month_wt1", np.float64),
                           ("month_wt2", np.float64)], align=True)
SERIES_FORCING = ("atm_tbot", "atm_pbot", "atm_qbot", "atm_flds", "atm_fsds", "atm_prec", "atm_wind")
SERIES_PHENOLOGY = ("mlai", "msai", "mhtop", "mhbot")

# member order of ELM::PFTDataPSN (src/data/pft_data.h:20-24)
PSN_FIELDS = (
    "fnr act25 kcha koha cpha vcmaxha jmaxha tpuha lmrha vcmaxhd jmaxhd tpuhd lmrhd lmrse qe theta_cj "
    "bbbopt mbbopt c3psn slatop leafcn flnr fnitr dleaf smpso smpsc tc_stress"
).split()
ALB_SOURCES = ["rholvis", "rholnir", "rhosvis", "rhosnir", "taulvis", "taulnir", "tausvis", "tausnir", "xl"]


def _p(a):
    """The address of a numpy array's data as the ABI's void pointer."""
    return a.ctypes.data_as(C.c_void_p)


def _csr_args(ptr, col, w, rows_name):
    """A CSR map as the ABI takes it: (nrows, ptr int64 [nrows + 1], col int32 [nnz], w float64 [nnz])."""
    ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
    col = np.ascontiguousarray(col, dtype=np.int32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if ptr.size < 2 or col.size != w.size or ptr[-1] != col.size:
        raise ValueError(f"ptr must be [{rows_name} + 1] with ptr[-1] == len(col) == len(w)")
    return ptr.size - 1, ptr, col, w


def field_table():
    lib = L.load()
    out = {}
    for i in range(lib.elmk_num_fields()):
        nlev, dt = C.c_int(), C.c_int()
        lib.elmk_field_info(i, C.byref(nlev), C.byref(dt))
        out[lib.elmk_field_name(i).decode()] = (i, nlev.value, DTYPES[dt.value])
    return out


def field_class(name, lib_path=None):
    """Restart class of a field (name or id), from the library's table."""
    lib = L.load(lib_path)
    fid = lib.elmk_field_id(name.encode()) if isinstance(name, str) else int(name)
    c = lib.elmk_field_class(fid)
    if c < 0:
        raise KeyError(name)
    return c


def pack_pft(pft):
    """PFTData::get_pft_psn / get_pft_alb (src/data/pft_data_impl.hh:64-116) for all 25 PFTs -> flat tables."""
    psn = np.zeros((25, 27))
    for j, name in enumerate(PSN_FIELDS):
        v = np.asarray(pft[name], dtype=np.float64).reshape(-1)
        psn[:, j] = v[0] if name == "tc_stress" else v[:25]
    alb = np.zeros((25, 9))
    for j, name in enumerate(ALB_SOURCES):
        alb[:, j] = np.asarray(pft[name], dtype=np.float64).reshape(-1)[:25]
    z0mr = np.ascontiguousarray(np.asarray(pft["z0mr"], dtype=np.float64).reshape(-1)[:25])
    displar = np.ascontiguousarray(np.asarray(pft["displar"], dtype=np.float64).reshape(-1)[:25])
    return psn, alb, z0mr, displar


class ELMState:
    def __init__(self, ncols, device=0, lib_path=None):
        self.lib = L.load(lib_path)
        self.ncols = int(ncols)
        self.device = int(device)
        h = C.c_void_p()
        rc = self.lib.elmk_create(self.ncols, self.device, C.byref(h))
        if rc != 0:
            raise L.ElmkError(f"elmk_create failed ({rc}): {self.lib.elmk_last_error(None).decode()}")
        self.ctx = h
        self.fields = field_table()
        self.scalars = dict(dewmx=0.1, oldfflag=1, dayl=0.0, max_dayl=0.0)
        self.land = dict(ltype=1, ctype=0, vtype=2, urbpoi=0, lakpoi=0)
        self._hist_nlev = {}  # history entry id -> levels of its field
        self._hist_cells = set()  # ids of gridded history entries (their results are cell-shaped)
        self._points_n, self._points_kind = [0, 0], {}  # point series: the two lists' sizes, entry id -> the list it samples
        self.output_ncells = None  # cells of the output grid (set_output_grid)
        self._accum_nlev = {}  # accumulator entry id -> levels of its source field

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.elmk_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc < 0:
            raise L.ElmkError(f"{what} failed ({rc}): {self.lib.elmk_last_error(self.ctx).decode()}")
        return rc

    def _ell_args(self, idx, w):
        """A per-column ELL map as the ABI takes it: (npts, idx int32 [npts, ncols], w float64 [npts, ncols])."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if idx.ndim == 1:
            idx, w = idx[None, :], w.reshape(1, -1)
        if idx.shape != w.shape or idx.shape[1] != self.ncols:
            raise ValueError(f"idx and w must both be [npts, {self.ncols}]")
        return idx.shape[0], idx, w

    # -- arrays -----------------------------------------------------------------------------------
    def upload(self, name, arr, col0=0, layout=LAYOUT_COL_MAJOR):
        fid, nlev, dt = self.fields[name]
        a = np.ascontiguousarray(arr, dtype=dt)
        n = a.size // nlev
        if a.size != n * nlev:
            raise ValueError(f"{name}: size {a.size} is not a multiple of nlev {nlev}")
        self._chk(self.lib.elmk_upload(self.ctx, fid, a.ctypes.data, col0, n, layout), f"upload({name})")

    def download(self, name, col0=0, n=None, layout=LAYOUT_COL_MAJOR, out=None):
        fid, nlev, dt = self.fields[name]
        n = self.ncols - col0 if n is None else n
        shape = (n,) if nlev == 1 else ((n, nlev) if layout == LAYOUT_COL_MAJOR else (nlev, n))
        if out is None:
            out = np.empty(shape, dtype=dt)
        assert out.shape == shape and out.dtype == dt and out.flags.c_contiguous
        self._chk(self.lib.elmk_download(self.ctx, fid, out.ctypes.data, col0, n, layout), f"download({name})")
        return out

    def __setitem__(self, name, arr):
        self.upload(name, arr)

    def __getitem__(self, name):
        return self.download(name)

    def fill(self, name, value):
        self._chk(self.lib.elmk_fill(self.ctx, self.fields[name][0], float(value)), f"fill({name})")

    def device_ptr(self, name):
        return self.lib.elmk_device_ptr(self.ctx, self.fields[name][0])

    @property
    def level_stride(self):
        return self.lib.elmk_level_stride(self.ctx)

    @property
    def device_bytes(self):
        return self.lib.elmk_device_bytes(self.ctx)

    def tile_columns(self, nbase, seed=0x5EEDE1A0, rules=()):
        """Replicate columns [0, nbase) over the rest of the state; rules = [(field, mode, amp)]."""
        arr = (L.Perturb * max(len(rules), 1))()
        for i, (name, mode, amp) in enumerate(rules):
            arr[i] = L.Perturb(self.fields[name][0], int(mode), float(amp))
        self._chk(
            self.lib.elmk_tile_columns(self.ctx, int(nbase), int(seed), len(rules), C.cast(arr, C.c_void_p)),
            "tile_columns",
        )

    def snapshot_fields(self, names):
        ids = (C.c_int * len(names))(*[self.fields[n][0] for n in names])
        self._chk(self.lib.elmk_snapshot_fields(self.ctx, ids, len(names)), "snapshot_fields")

    def restore_fields(self):
        self._chk(self.lib.elmk_restore_fields(self.ctx), "restore_fields")

    # -- parameters -------------------------------------------------------------------------------
    def set_land(self, **kw):
        self.land.update(kw)
        l = self.land
        self._chk(
            self.lib.elmk_set_land(self.ctx, int(l["ltype"]), int(l["ctype"]), int(l["vtype"]), int(l["urbpoi"]), int(l["lakpoi"])),
            "set_land",
        )

    def set_scalars(self, **kw):
        self.scalars.update(kw)
        s = self.scalars
        self._chk(
            self.lib.elmk_set_scalars(self.ctx, float(s["dewmx"]), int(s["oldfflag"]), float(s["dayl"]), float(s["max_dayl"])),
            "set_scalars",
        )

    def set_pft(self, pft):
        psn, alb, z0mr, displar = pack_pft(pft)
        self.set_pft_tables(psn, alb, z0mr, displar)

    def set_pft_tables(self, psn, alb, z0mr, displar):
        a = [np.ascontiguousarray(x, dtype=np.float64) for x in (psn, alb, z0mr, displar)]
        assert a[0].shape == (25, 27) and a[1].shape == (25, 9) and a[2].shape == (25,) and a[3].shape == (25,)
        self._chk(self.lib.elmk_set_pft(self.ctx, *[x.ctypes.data for x in a]), "set_pft")

    def set_soilcolor(self, albsat, albdry):
        a = np.ascontiguousarray(albsat, dtype=np.float64)
        b = np.ascontiguousarray(albdry, dtype=np.float64)
        assert a.shape == (20, 2) and b.shape == (20, 2)
        self._chk(self.lib.elmk_set_soilcolor(self.ctx, a.ctypes.data, b.ctypes.data), "set_soilcolor")

    def set_snicar(self, tables):
        keep = []
        t = L.SnicarTables()
        for name in L.SNICAR_NAMES:
            a = np.ascontiguousarray(np.asarray(tables[name], dtype=np.float64).reshape(-1))
            if a.size != L.SNICAR_SIZES[name]:
                raise ValueError(f"snicar table {name}: {a.size} values, expected {L.SNICAR_SIZES[name]}")
            keep.append(a)
            setattr(t, name, a.ctypes.data)
        self._chk(self.lib.elmk_set_snicar(self.ctx, C.byref(t)), "set_snicar")

    def set_init_params(self, organic_max, roota_par, rootb_par):
        """organic_max of the parameter file (initialize_elm_kokkos.cc:312) and PFTData::roota_par / rootb_par [25]."""
        a = np.ascontiguousarray(roota_par, dtype=np.float64)
        b = np.ascontiguousarray(rootb_par, dtype=np.float64)
        assert a.shape == (25,) and b.shape == (25,)
        self._chk(self.lib.elmk_set_init_params(self.ctx, float(organic_max), _p(a), _p(b)), "set_init_params")

    def set_snow_age_tables(self, tables):
        """SnwRdsTable: tables [3, 11, 31, 8] = snowage_tau, snowage_kappa, snowage_drdt0."""
        t = np.ascontiguousarray(tables, dtype=np.float64)
        assert t.shape == (3, 11, 31, 8)
        self._chk(self.lib.elmk_set_snow_age_tables(self.ctx, *[_p(t[k]) for k in range(3)]), "set_snow_age_tables")

    # -- control ----------------------------------------------------------------------------------
    def sync(self):
        self._chk(self.lib.elmk_sync(self.ctx), "sync")

    def set_stream(self, hip_stream_handle):
        self._chk(self.lib.elmk_set_stream(self.ctx, C.c_void_p(hip_stream_handle or 0)), "set_stream")

    def error_summary(self):
        flags, first = C.c_uint32(), C.c_int64()
        self._chk(self.lib.elmk_error_summary(self.ctx, C.byref(flags), C.byref(first)), "error_summary")
        return flags.value, first.value

    def clear_errors(self):
        self._chk(self.lib.elmk_clear_errors(self.ctx), "clear_errors")

    def profile_timestep7(self, dt, nsteps):
        ms = (C.c_float * 7)()
        tot = C.c_float()
        self._chk(self.lib.elmk_profile_timestep7(self.ctx, float(dt), int(nsteps), ms, C.byref(tot)), "profile_timestep7")
        return list(ms), tot.value

    def profile_timestep7_fused(self, dt, nsteps):
        ms = (C.c_float * len(KERNEL_NAMES_FUSED))()
        tot = C.c_float()
        self._chk(self.lib.elmk_profile_timestep7_fused(self.ctx, float(dt), int(nsteps), ms, C.byref(tot)), "profile_timestep7_fused")
        return list(ms), tot.value

    def profile_steps(self, dt, nsteps, fused=False):
        """Device time (ms) of each of nsteps steps (HIP events around every step; snapshot restored before each)."""
        ms = (C.c_float * int(nsteps))()
        self._chk(self.lib.elmk_profile_steps(self.ctx, int(bool(fused)), float(dt), int(nsteps), ms), "profile_steps")
        return list(ms)

    def canopy_trip_counts(self):
        """Trips of the leaf-temperature iteration per column in the last canopy_fluxes call (0: not vegetated)."""
        out = np.zeros(self.ncols, dtype=np.int32)
        self._chk(self.lib.elmk_read_scratch(self.ctx, 0, _p(out), 0, self.ncols), "read_scratch")
        return out

    def canopy_schedule_hints(self):
        """The scheduler's hint per column: slowly decaying maximum of the trip count (development diagnostics)."""
        out = np.zeros(self.ncols, dtype=np.int32)
        self._chk(self.lib.elmk_read_scratch(self.ctx, 2, _p(out), 0, self.ncols), "read_scratch")
        return out

    def work_list_counters(self):
        """(entries, queue head) of every internal work list [nlists, 2]: all zero between two wrapper calls."""
        n = 8
        out = np.zeros(2 * n, dtype=np.uint32)
        self._chk(self.lib.elmk_read_scratch(self.ctx, 3, _p(out), 0, 2 * n), "read_scratch")
        return out.reshape(n, 2)

    def read_work(self, offset, count):
        out = np.zeros(int(count), dtype=np.float64)
        self._chk(self.lib.elmk_read_scratch(self.ctx, 1, _p(out), int(offset), int(count)), "read_scratch")
        return out

    def profile_wrapper(self, wrapper, dt, nsteps=5):
        """Mean device time (ms, HIP events on the launch stream) of one wrapper; wrapper: index into WRAPPER_NAMES."""
        ms = C.c_float()
        self._chk(self.lib.elmk_profile_wrapper(self.ctx, int(wrapper), float(dt), int(nsteps), C.byref(ms)), "profile_wrapper")
        return ms.value

    def set_option(self, option, value):
        """Launch options (elmk_set_option); OPT_CF_HALF_WORKGROUPS: the leaf-temperature iteration in 256-thread workgroups, one per CU;
        OPT_ALB_STAGED: albedo_snicar's one-layer SNICAR and final stage as launches of their own instead of k_alb_tile;
        OPT_RESTART_CELLS: restart_save / restart_load of a context with the routing enabled carry the river stages' state (VOLR,
        QOUT_SUM and the call count, WH, WT, WF, UNMET_SUM): no routing_init / ..._init call after a load."""
        self._chk(self.lib.elmk_set_option(self.ctx, int(option), int(value)), "set_option")

    def set_graph(self, on=True):
        """timestep7 as one replayed HIP graph (elmk_set_graph)."""
        self._chk(self.lib.elmk_set_graph(self.ctx, int(bool(on))), "set_graph")

    def copy_bandwidth(self, nbytes=1 << 30, iters=20, shape=0):
        """device-to-device copy rate in GB/s (read + write bytes); shape: see elmk_copy_bandwidth_shape"""
        g = C.c_double()
        self._chk(self.lib.elmk_copy_bandwidth_shape(self.ctx, int(nbytes), int(iters), int(shape), C.byref(g)), "copy_bandwidth")
        return g.value


    # -- per-column solar geometry (include/elmk.h: elmk_set_column_geography ...) -------------------
    def set_column_geography(self, lat, lon):
        """Latitude and longitude of every column, radians ([ncols] each; |lat| <= pi/2 + 10 eps).  Changes nothing until
        solar_geometry() runs."""
        lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
        lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
        assert lat.size == self.ncols and lon.size == self.ncols
        self._chk(self.lib.elmk_set_column_geography(self.ctx, _p(lat), _p(lon)), "set_column_geography")

    def solar_geometry(self, dt, decday, doy):
        """kokkos_init_timestep's solar lines for every column at its own location: coszen, and per-column day length for
        canopy_fluxes from now on (decday = decimal_doy(date) + 1.0, doy = date.doy)."""
        self._chk(self.lib.elmk_solar_geometry(self.ctx, float(dt), float(decday), int(doy)), "solar_geometry")

    def day_length(self):
        """(dayl, max_dayl) of every column from the last solar_geometry()."""
        dayl, max_dayl = np.empty(self.ncols), np.empty(self.ncols)
        self._chk(self.lib.elmk_download_day_length(self.ctx, _p(dayl), _p(max_dayl)), "day_length")
        return dayl, max_dayl

    def clear_column_geography(self):
        """Back to one day length for all columns (set_scalars' dayl / max_dayl)."""
        self._chk(self.lib.elmk_clear_column_geography(self.ctx), "clear_column_geography")

    # -- history (include/elmk.h: elmk_history_add ...) ---------------------------------------------
    def history_add(self, tape, name, op):
        """Register every level of field `name` on `tape` with op ("avg", "sum", "max", "min", "inst" or HIST_*); returns the
        entry id.  Refused (ElmkError) for an unknown field / op / tape, a full table, a tape holding samples, a stream in capture."""
        fid = self.fields[name][0] if isinstance(name, str) else int(name)
        code = HIST_OPS[op] if isinstance(op, str) else int(op)
        entry = self._chk(self.lib.elmk_history_add(self.ctx, int(tape), fid, code), f"history_add({name})")
        nlev = C.c_int()
        self.lib.elmk_field_info(fid, C.byref(nlev), None)
        self._hist_nlev[entry] = nlev.value
        return entry

    def history_add_row(self, tape, family, which, op):
        """As history_add over one fp64 row of a feature instead of a state field: family "alt", "hydrology", "frost" or
        "water_balance" (or ROWS_*), which the family's row number (ALT_*, hydrology.ZWT .., hydrology.FROST_TABLE ..,
        hydrology.WB_*).  One level; refused as history_add, and for a family that is not enabled or a row out of range.  While the
        entry exists the family's clear is refused (history_clear first)."""
        fam = ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        code = HIST_OPS[op] if isinstance(op, str) else int(op)
        entry = self._chk(self.lib.elmk_column_history_add_row(self.ctx, int(tape), fam, int(which), code), f"history_add_row({family}, {which})")
        self._hist_nlev[entry] = 1
        return entry

    def history_accumulate(self):
        """Fold the current state into every tape's accumulators and count one sample per tape with entries: one launch, no sync."""
        self._chk(self.lib.elmk_history_accumulate(self.ctx), "history_accumulate")

    def history_reset(self, tape):
        """The tape's accumulators back to their initial values, its count to 0 (stream-ordered)."""
        self._chk(self.lib.elmk_history_reset(self.ctx, int(tape)), "history_reset")

    def history_count(self, tape):
        n = C.c_int64()
        self._chk(self.lib.elmk_history_count(self.ctx, int(tape), C.byref(n)), "history_count")
        return n.value

    def history_read(self, entry, col0=0, n=None, layout=LAYOUT_COL_MAJOR, nlev=None):
        """The entry's result as float64: [n] for a one-level field, else [n, nlev] (COL_MAJOR) or [nlev, n] (SOA).  For a gridded
        entry (gridded_history_add) col0 and n index cells of the output grid (n defaults to the cells from col0 on)."""
        if n is None:
            n = (self.output_ncells if int(entry) in self._hist_cells else self.ncols) - col0
        n = int(n)
        if nlev is None:
            nlev = self._hist_nlev.get(int(entry), 1)
        shape = (n,) if nlev == 1 else ((n, nlev) if layout == LAYOUT_COL_MAJOR else (nlev, n))
        out = np.empty(shape, dtype=np.float64)
        self._chk(self.lib.elmk_history_read(self.ctx, int(entry), _p(out), int(col0), n, int(layout)), "history_read")
        return out

    def history_clear(self):
        """Drop every entry of every tape and free its device buffers."""
        self._chk(self.lib.elmk_history_clear(self.ctx), "history_clear")
        self._hist_nlev.clear()
        self._hist_cells.clear()

    # -- accumulated fields (include/elmk.h: elmk_accum_add ...; elmkernels_amd/accum.py restates the update) ------------------
    def accum_add(self, src, kind, period_steps, dst=None):
        """Register an accumulated field over every level of field `src`: kind "runmean", "timeavg", "runaccum" or ACCUM_*, the
        period in steps, `dst` the field that receives the value (or None).  Returns the entry id.  Refused (ElmkError) for an unknown
        field or kind, a period < 1, a destination that is not an F64 SURFACE field of the source's levels, that another entry writes
        or that is the source, a full table, a stream in capture."""
        sid = self.fields[src][0] if isinstance(src, str) else int(src)
        did = -1 if dst is None else (self.fields[dst][0] if isinstance(dst, str) else int(dst))
        code = ACCUM_KINDS[kind] if isinstance(kind, str) else int(kind)
        entry = self._chk(self.lib.elmk_accum_add(self.ctx, sid, code, int(period_steps), did), f"accum_add({src})")
        nlev = C.c_int()
        self.lib.elmk_field_info(sid, C.byref(nlev), None)
        self._accum_nlev[entry] = nlev.value
        return entry

    def accum_init(self, entry, values=None, nsteps=0):
        """Set the entry's value from values ([ncols] or [nlev, ncols], SoA) and its step count (a restart file's T10 and nstep);
        values None: seeded from the destination field's current contents.  Synchronises."""
        p = None
        if values is not None:
            a = np.ascontiguousarray(values, dtype=np.float64)
            if a.size != self._accum_nlev.get(int(entry), 1) * self.ncols:
                raise ValueError(f"accum_init: {a.size} values for {self._accum_nlev.get(int(entry), 1)} x {self.ncols}")
            p = _p(a)
        self._chk(self.lib.elmk_accum_init(self.ctx, int(entry), p, int(nsteps)), "accum_init")

    def accum_update(self):
        """Fold the current state into every accumulated field and write the destinations: stream-ordered, no sync."""
        self._chk(self.lib.elmk_accum_update(self.ctx), "accum_update")

    def accum_read(self, entry, col0=0, n=None, layout=LAYOUT_SOA):
        """(val, nsteps): the entry's fp64 value - [n] for a one-level source, else [nlev, n] (SOA) or [n, nlev] (COL_MAJOR) - and
        the updates folded in so far.  Synchronises."""
        n = int(self.ncols - col0 if n is None else n)
        nlev = self._accum_nlev.get(int(entry), 1)
        shape = (n,) if nlev == 1 else ((n, nlev) if layout == LAYOUT_COL_MAJOR else (nlev, n))
        out = np.empty(shape, dtype=np.float64)
        cnt = C.c_int64()
        self._chk(self.lib.elmk_accum_read(self.ctx, int(entry), _p(out), int(col0), n, int(layout), C.byref(cnt)), "accum_read")
        return out, cnt.value

    def accum_clear(self):
        """Drop every accumulated field and free its device buffers (destination fields keep their values)."""
        self._chk(self.lib.elmk_accum_clear(self.ctx), "accum_clear")
        self._accum_nlev.clear()

    # -- active layer thickness (include/elmk.h: elmk_active_layer_enable ...; elmkernels_amd/active_layer.py restates the update) --
    def active_layer_enable(self):
        """Allocate the rows alt, altmax, altmax_lastyear (fp64, zero-filled); the index fields altmax_indx and
        altmax_lastyear_indx keep what was uploaded.  Refused when already enabled or while the stream is captured."""
        self._chk(self.lib.elmk_active_layer_enable(self.ctx), "active_layer_enable")

    def active_layer_init(self, altmax=None, altmax_lastyear=None):
        """altmax and altmax_lastyear from [ncols] each (None: zeros), alt = zeros: a restart file's ALTMAX.  Synchronises."""
        self._init_rows("active_layer_init", (altmax, altmax_lastyear), "columns")

    def _init_rows(self, name, rows, unit, *more):
        """elmk_<name>(ctx, rows ..., more ...): each row an optional array (None: the call's default) of one value per column
        (unit "columns") or per routing cell ("cells")."""
        n = self.ncols if unit == "columns" else getattr(self, "routing_ncells", None)
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in rows]
        for v in a:
            if v is not None and n is not None and v.size != n:
                raise ValueError(f"{name}: {v.size} values for {n} {unit}")
        self._chk(getattr(self.lib, "elmk_" + name)(self.ctx, *(None if v is None else _p(v) for v in a), *more), name)

    def _read_row(self, name, which, i0, n, total, clamp=False):
        """elmk_<name>(ctx, which, out, i0, n): float64 [n] of row `which` from index i0 on; n None: the rest of `total`.  clamp: a
        negative n is left to the entry point to refuse (otherwise numpy refuses it)."""
        n = int(total - i0 if n is None else n)
        out = np.empty(max(n, 0) if clamp else n, dtype=np.float64)
        self._chk(getattr(self.lib, "elmk_" + name)(self.ctx, int(which), _p(out), int(i0), n), name)
        return out

    # -- irrigation (include/elmk.h: elmk_irrigation_enable ...; elmkernels_amd/irrigation.py restates the stage) ---------------------
    def irrigation_enable(self, sched):
        """Allocate the rows RATE, NLEFT, QFLX_IRRIG (fp64, zero-filled) and the parameter row sched: int32 [ncols], -1 = not irrigated,
        else the longitude offset in seconds 0 .. 86399 (irrigation.schedule).  Refused when already enabled, for a value outside
        -1 .. 86399, while the stream is captured."""
        s = np.ascontiguousarray(sched, dtype=np.int32).reshape(-1)
        if s.size != self.ncols:
            raise ValueError(f"irrigation_enable: {s.size} values for {self.ncols} columns")
        self._chk(self.lib.elmk_irrigation_enable(self.ctx, _p(s)), "irrigation_enable")

    def irrigation_init(self, rate=None, nleft=None):
        """RATE and NLEFT from [ncols] each (None: zeros), QFLX_IRRIG = zeros: a restart file's values.  Synchronises."""
        self._init_rows("irrigation_init", (rate, nleft), "columns")

    def irrigation(self, dt, tod):
        """The stage: apply, then check.  After timestep7 / timestep7_fused, before soil_temperature; one launch, stream-ordered, no
        sync.  dt: a whole number of seconds in 1 .. 86400; tod: seconds after midnight UTC at the step's start (irrigation.time_of_day)."""
        self._chk(self.lib.elmk_irrigation(self.ctx, float(dt), int(tod)), "irrigation")

    def irrigation_read(self, which, col0=0, n=None):
        """Row IRR_RATE, IRR_NLEFT or IRR_QFLX_IRRIG of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("irrigation_read", which, col0, n, self.ncols, clamp=True)

    def irrigation_rows(self):
        """Every row of the feature: float64 [IRR_NROWS, ncols], the `rows` of irrigation.step."""
        return np.stack([self.irrigation_read(w) for w in range(IRR_NROWS)])

    def irrigation_clear(self):
        """Free the rows and sched.  Refused while history entries over the rows exist."""
        self._chk(self.lib.elmk_irrigation_clear(self.ctx), "irrigation_clear")

    # -- the irrigation's river supply limit (include/elmk.h: elmk_irrigation_supply_enable ...; irrigation.supply_limit restates it) ----
    def irrigation_supply_enable(self, threshold=0.1):
        """Limit every demand check by the channel storage of the column's cell: from here on irrigation() and the irrigation stage of
        run() enqueue the limiter behind the irrigation.  Allocates the cell rows DEMAND, COMMITTED, RATIO, UNMET_SUM (fp64, zero-filled).
        Needs irrigation_enable, routing_enable with routing_set_withdrawal(True), 0 <= threshold < 1 and an output grid in which every
        column lies in at most one cell."""
        self._chk(self.lib.elmk_irrigation_supply_enable(self.ctx, float(threshold)), "irrigation_supply_enable")

    def irrigation_supply_init(self, unmet_sum=None):
        """UNMET_SUM from [ncells] (None: zeros), the other rows zeros: a restart file's values.  Synchronises."""
        self._init_rows("irrigation_supply_init", (unmet_sum,), "cells")

    def irrigation_supply_read(self, which, cell0=0, n=None):
        """Row IRRSUP_DEMAND, IRRSUP_COMMITTED, IRRSUP_RATIO or IRRSUP_UNMET_SUM of cells [cell0, cell0 + n): float64 [n].  Synchronises."""
        return self._read_row("irrigation_supply_read", which, cell0, n, getattr(self, "routing_ncells", 0), clamp=True)

    def irrigation_supply_rows(self):
        """Every row of the limit: float64 [IRRSUP_NROWS, ncells]."""
        return np.stack([self.irrigation_supply_read(w) for w in range(IRRSUP_NROWS)])

    def irrigation_supply_reset(self):
        """UNMET_SUM = zeros (stream-ordered)."""
        self._chk(self.lib.elmk_irrigation_supply_reset(self.ctx), "irrigation_supply_reset")

    def irrigation_supply_clear(self):
        """Switch the limit off and free its rows."""
        self._chk(self.lib.elmk_irrigation_supply_clear(self.ctx), "irrigation_supply_clear")

    # -- runoff routing (include/elmk.h: elmk_routing_enable ...; elmkernels_amd/routing.py restates the stage) ---------------------------
    def routing_enable(self, down, ddist, area, effvel=0.35, nsub=1):
        """Allocate the cell rows VOLR, QIN, QOUT, QOUT_SUM (fp64, zero-filled) over the output grid's cells and take the network: down
        int32 [ncells] (-1 = an outlet), ddist [ncells] metres, area [ncells] square metres, effvel m/s, nsub sub-steps per call.  Needs
        an output grid and the water balance.  Refused for a network that is out of range, has a self-loop, a cycle or more than 8 cells
        draining into one, and while the stream is captured."""
        d = np.ascontiguousarray(down, dtype=np.int32).reshape(-1)
        dd = np.ascontiguousarray(ddist, dtype=np.float64).reshape(-1)
        a = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
        if not (d.size == dd.size == a.size):
            raise ValueError("routing_enable: down, ddist and area must all be [ncells]")
        self._chk(self.lib.elmk_routing_enable(self.ctx, int(d.size), _p(d), _p(dd), _p(a), float(effvel), int(nsub)), "routing_enable")
        self.routing_ncells = int(d.size)

    def routing_init(self, volr=None, qout_sum=None, ncalls=0):
        """VOLR and QOUT_SUM from [ncells] each (None: zeros), QIN and QOUT zeros, the call count = ncalls: a restart file's values.
        Synchronises."""
        self._init_rows("routing_init", (volr, qout_sum), "cells", int(ncalls))

    def _routing_budget(self, name, n):
        """elmk_<name>(ctx, sums): float64 [n]."""
        out = np.empty(n, dtype=np.float64)
        self._chk(getattr(self.lib, "elmk_" + name)(self.ctx, _p(out)), name)
        return out

    def routing(self, dt):
        """One call: QIN from the water balance's QRUNOFF row, then nsub sub-steps.  After water_balance(dt); nsub + 1 launches,
        stream-ordered, no sync."""
        self._chk(self.lib.elmk_routing(self.ctx, float(dt)), "routing")

    def routing_read(self, which, cell0=0, n=None):
        """Row ROUTE_VOLR, ROUTE_QIN, ROUTE_QOUT or ROUTE_QOUT_SUM (with the kinematic-wave scheme on also ROUTE_WH, ROUTE_WT, ROUTE_QSUR,
        with its floodplain inundation on also ROUTE_WF, ROUTE_FLOOD_DEPTH, ROUTE_FLOOD_FRAC, with its reservoirs on also ROUTE_RES,
        ROUTE_KRLS, ROUTE_RES_TAKE, with its stream temperature on also ROUTE_TT .. ROUTE_HOUT, with the command areas on also
        ROUTE_CMD_WANT .. ROUTE_CMD_RATIO)
        of cells [cell0, cell0 + n): float64 [n].  Synchronises."""
        return self._read_row("routing_read", which, cell0, n, getattr(self, "routing_ncells", 0), clamp=True)

    def routing_count(self):
        """The calls since the last routing_init / routing_reset_mean: routing_read(ROUTE_QOUT_SUM) / routing_count() is the mean."""
        n = C.c_int64(0)
        self._chk(self.lib.elmk_routing_count(self.ctx, C.byref(n)), "routing_count")
        return int(n.value)

    def routing_reset_mean(self):
        self._chk(self.lib.elmk_routing_reset_mean(self.ctx), "routing_reset_mean")

    def routing_set_withdrawal(self, on=True):
        """on: every call takes the irrigation's applied water out of the cells' input (needs irrigation_enable)."""
        self._chk(self.lib.elmk_routing_set_withdrawal(self.ctx, 1 if on else 0), "routing_set_withdrawal")

    def routing_budget(self):
        """float64 [3]: the sums of VOLR and QIN and the sum of QOUT over the outlets (routing.budget).  Synchronises."""
        return self._routing_budget("routing_budget", 3)

    def routing_clear(self):
        self._chk(self.lib.elmk_routing_clear(self.ctx), "routing_clear")

    # -- kinematic-wave routing (include/elmk.h: elmk_routing_kinematic_enable ...; routing.kinematic_call restates the scheme) -----------
    def routing_kinematic_enable(self, params):
        """Switch the routing stage to the kinematic-wave scheme: params float64 [ROUTE_KW_NPARAM, ncells] in the order of routing.HSLP ..
        routing.NR, every value finite and > 0.  Allocates the rows WH, WT, QSUR (zero-filled); routing_read takes ROUTE_WH, ROUTE_WT and
        ROUTE_QSUR from here on.  Needs routing_enable and soil_hydrology_enable."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        n = getattr(self, "routing_ncells", None)
        if n is not None and p.shape != (ROUTE_KW_NPARAM, n):
            raise ValueError(f"routing_kinematic_enable: params must be [{ROUTE_KW_NPARAM}, {n}]")
        self._chk(self.lib.elmk_routing_kinematic_enable(self.ctx, _p(p)), "routing_kinematic_enable")

    def routing_kinematic_init(self, wh=None, wt=None):
        """WH and WT from [ncells] each (None: zeros), QSUR zeros; VOLR, QOUT_SUM and the count stay routing_init's.  Synchronises."""
        self._init_rows("routing_kinematic_init", (wh, wt), "cells")

    def routing_kinematic_budget(self):
        """float64 [2]: the sums of WH and WT (routing.kinematic_budget).  Synchronises."""
        return self._routing_budget("routing_kinematic_budget", 2)

    def routing_kinematic_clear(self):
        """Back to the linear scheme; VOLR, QOUT_SUM and the count stay."""
        self._chk(self.lib.elmk_routing_kinematic_clear(self.ctx), "routing_kinematic_clear")

    # -- floodplain inundation (include/elmk.h: elmk_routing_inundation_enable ...; routing.inundation_exchange restates it) ---------------
    def routing_inundation_enable(self, rdepth, eprof):
        """Give the kinematic scheme's main channel banks and a floodplain: rdepth float64 [ncells], the bank height in metres (finite
        and > 0), eprof float64 [ROUTE_FP_NPROF, ncells], the elevation above the bank top at which the fraction k / 10 of the
        floodplain is wet (finite, eprof[0] == 0, strictly increasing).  Allocates the rows WF, FLOOD_DEPTH, FLOOD_FRAC (zero-filled);
        routing_read takes ROUTE_WF, ROUTE_FLOOD_DEPTH and ROUTE_FLOOD_FRAC from here on.  Needs routing_kinematic_enable."""
        r = np.ascontiguousarray(rdepth, dtype=np.float64).reshape(-1)
        e = np.ascontiguousarray(eprof, dtype=np.float64)
        n = getattr(self, "routing_ncells", r.size)
        if r.size != n or e.shape != (ROUTE_FP_NPROF, n):
            raise ValueError(f"routing_inundation_enable: rdepth must be [{n}] and eprof [{ROUTE_FP_NPROF}, {n}]")
        self._chk(self.lib.elmk_routing_inundation_enable(self.ctx, _p(r), _p(e)), "routing_inundation_enable")

    def routing_inundation_init(self, wf=None):
        """WF from [ncells] (None: zeros), the two diagnostics zeros; VOLR, WH and WT stay their own entries'.  Synchronises."""
        self._init_rows("routing_inundation_init", (wf,), "cells")

    def routing_inundation_budget(self):
        """float64 [1]: the sum of WF (routing.inundation_budget).  Synchronises."""
        return self._routing_budget("routing_inundation_budget", 1)

    def routing_inundation_clear(self):
        """Back to the channel without banks; WF is dropped, VOLR stays."""
        self._chk(self.lib.elmk_routing_inundation_clear(self.ctx), "routing_inundation_clear")

    # -- reservoirs (include/elmk.h: elmk_routing_reservoir_enable ...; routing.kinematic_call(dam=) restates them) -------------------------
    def routing_reservoir_enable(self, cap, target, beta, mstart):
        """Put dams at the outlets of the kinematic scheme's cells: cap float64 [ncells], m3 (finite and >= 0; 0 = no dam), target float64
        [12, ncells], the monthly target release in m3/s (finite and >= 0), beta float64 [ncells] in [0, 1], mstart int32 [ncells] in
        0 .. 11; the last three are checked only where cap > 0.  Allocates the rows RES, RES_TAKE (zero-filled) and KRLS (1.0);
        routing_read takes ROUTE_RES, ROUTE_KRLS and ROUTE_RES_TAKE from here on.  Needs routing_kinematic_enable."""
        c = np.ascontiguousarray(cap, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(target, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        m = np.ascontiguousarray(mstart, dtype=np.int32).reshape(-1)
        n = getattr(self, "routing_ncells", c.size)
        if c.size != n or t.shape != (12, n) or b.size != n or m.size != n:
            raise ValueError(f"routing_reservoir_enable: cap, beta and mstart must be [{n}] and target [12, {n}]")
        self._chk(self.lib.elmk_routing_reservoir_enable(self.ctx, _p(c), _p(t), _p(b), _p(m)), "routing_reservoir_enable")

    def routing_reservoir_init(self, res=None, krls=None):
        """RES from [ncells] (None: zeros), KRLS from [ncells] (None: 1.0), RES_TAKE zeros.  Synchronises."""
        self._init_rows("routing_reservoir_init", (res, krls), "cells")

    def routing_reservoir_time(self, month, begins=False):
        """The month (0 .. 11) of the following routing() calls, and whether the next one is the call whose step starts at 00:00 of the
        month's first day (routing.month_of_doy); run() derives both from its steps."""
        self._chk(self.lib.elmk_routing_reservoir_time(self.ctx, int(month), 1 if begins else 0), "routing_reservoir_time")

    def routing_reservoir_budget(self):
        """float64 [2]: the sums of RES and RES_TAKE (routing.reservoir_budget).  Synchronises."""
        return self._routing_budget("routing_reservoir_budget", 2)

    def routing_reservoir_clear(self):
        """Back to the free-flowing channel; RES is dropped, VOLR stays."""
        self._chk(self.lib.elmk_routing_reservoir_clear(self.ctx), "routing_reservoir_clear")

    # -- command areas (include/elmk.h: elmk_routing_command_enable ...; routing.kinematic_call(dam={..., "command": cmd}) restates them) ---
    def routing_command_enable(self, dam, share, claim):
        """Let the dams supply the cells that depend on them: dam int32 [ROUTE_CMD_NDEP, ncells], the cell of a supplying dam or -1 for an
        empty slot (filled from slot 0 without gaps), share float64 [ROUTE_CMD_NDEP, ncells] in (0, 1], the fraction of the cell's remaining
        withdrawal asked of that dam, claim float64 [ROUTE_CMD_NDEP, ncells] in [0, 1], the cell's right to the dam's usable storage at
        the supply limit's daily check (routing.check_command says the rest).  Allocates the rows ROUTE_CMD_WANT, _TAKE, _GIVE
        (zero-filled) and _RATIO (1.0); routing_read takes them from here on.  Needs routing_reservoir_enable and
        routing_set_withdrawal(True)."""
        d = np.ascontiguousarray(dam, dtype=np.int32)
        s = np.ascontiguousarray(share, dtype=np.float64)
        c = np.ascontiguousarray(claim, dtype=np.float64)
        n = getattr(self, "routing_ncells", d.shape[-1] if d.ndim == 2 else 0)
        if d.shape != (ROUTE_CMD_NDEP, n) or s.shape != d.shape or c.shape != d.shape:
            raise ValueError(f"routing_command_enable: dam, share and claim must be [{ROUTE_CMD_NDEP}, {n}]")
        self._chk(self.lib.elmk_routing_command_enable(self.ctx, _p(d), _p(s), _p(c)), "routing_command_enable")

    def routing_command_budget(self):
        """float64 [2]: the sums of CMD_GIVE and CMD_TAKE (routing.command_budget).  Synchronises."""
        return self._routing_budget("routing_command_budget", 2)

    def routing_command_clear(self):
        """Back to dams that serve their own cell only; RES stays."""
        self._chk(self.lib.elmk_routing_command_clear(self.ctx), "routing_command_clear")

    # -- stream temperature (include/elmk.h: elmk_routing_heat_enable ...; routing.kinematic_call(heat=) restates it) ------------------------
    def routing_heat_enable(self, sublev=0, shade=None):
        """Give the tributary store and the main channel of the kinematic scheme's cells a temperature: sublev 0 .. 14, the soil layer
        whose temperature the subsurface runoff carries; shade float64 [ncells] in [0, 1], the share of shortwave kept off the water
        (None: 0).  Allocates the rows TT and TR (273.15 K) and the five diagnostics; routing_read takes ROUTE_TT .. ROUTE_HOUT from
        here on.  Needs routing_kinematic_enable, and neither the inundation nor the reservoirs."""
        s = None if shade is None else np.ascontiguousarray(shade, dtype=np.float64).reshape(-1)
        if s is not None and s.size != getattr(self, "routing_ncells", s.size):
            raise ValueError(f"routing_heat_enable: {s.size} shade values for {self.routing_ncells} cells")
        self._chk(self.lib.elmk_routing_heat_enable(self.ctx, int(sublev), None if s is None else _p(s)), "routing_heat_enable")

    def routing_heat_init(self, tt=None, tr=None):
        """TT and TR from [ncells] (None: 273.15 K), the diagnostics zeros.  Synchronises."""
        self._init_rows("routing_heat_init", (tt, tr), "cells")

    def routing_heat_budget(self):
        """float64 [5]: the sums of HEAT, HIN, HSRF, HADJ and of HOUT over the outlets (routing.heat_budget).  Synchronises."""
        return self._routing_budget("routing_heat_budget", 5)

    def routing_heat_clear(self):
        """Back to the scheme without temperatures; TT and TR are dropped, the water stays."""
        self._chk(self.lib.elmk_routing_heat_clear(self.ctx), "routing_heat_clear")

    # -- floodplain infiltration (include/elmk.h: elmk_floodplain_infiltration_enable ...; hydrology.step(rof=), water_balance_end(
    #    qflx_h2orof_drain=) and routing.kinematic_call(land=) restate it) -------------------------------------------------------------
    def floodplain_infiltration_enable(self):
        """Let the floodplain's water infiltrate the soil columns of its cell: the soil hydrology, the water balance and the routing take
        their forms with the term from here on.  Allocates the column rows FPI_H2OROF, FPI_FRAC, FPI_QFLX_DRAIN and the cell row
        ROUTE_QLAND (zero-filled).  Needs soil_hydrology_enable, water_balance_enable, routing_kinematic_enable,
        routing_inundation_enable and an output grid with every column in at most one cell."""
        self._chk(self.lib.elmk_floodplain_infiltration_enable(self.ctx), "floodplain_infiltration_enable")

    def floodplain_infiltration_read(self, which, col0=0, n=None):
        """Row FPI_H2OROF, FPI_FRAC or FPI_QFLX_DRAIN of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("floodplain_infiltration_read", which, col0, n, self.ncols)

    def floodplain_infiltration_budget(self):
        """float64 [1]: the sum of QLAND (routing.land_budget).  Synchronises."""
        return self._routing_budget("floodplain_infiltration_budget", 1)

    def floodplain_infiltration_clear(self):
        """Back to the stages without the term; WF stays."""
        self._chk(self.lib.elmk_floodplain_infiltration_clear(self.ctx), "floodplain_infiltration_clear")

    # -- water balance (include/elmk.h: elmk_water_balance_enable ...; hydrology.water_balance_begin / _end restate the stage) -----
    def water_balance_enable(self, tol_mm):
        """Allocate the rows BEGWB .. TOTSOILICE and the reduction's scratch; tol_mm: a column is bad iff !(|ERRH2O| <= tol_mm).  Needs
        the soil hydrology; refused when already enabled, for a tolerance that is not finite and >= 0, while the stream is captured."""
        self._chk(self.lib.elmk_water_balance_enable(self.ctx, float(tol_mm)), "water_balance_enable")

    def water_balance_begin(self):
        """W0: BEGWB = dtbegin_column_h2o + WA.  After init_timestep, before the physics; one launch, no synchronisation."""
        self._chk(self.lib.elmk_water_balance_begin(self.ctx), "water_balance_begin")

    def water_balance(self, dt, read=True):
        """W1 - W8 after the step's soil_hydrology.  read=True synchronises and returns ((min, max, sum) [3, 3] of ERRH2O, QRUNOFF,
        ENDWB, nbad, first_bad_col); read=False only enqueues (capturable) and returns None."""
        if not read:
            self._chk(self.lib.elmk_water_balance(self.ctx, float(dt), None, None, None), "water_balance")
            return None
        mms, nbad, first = np.zeros((3, 3)), C.c_int64(), C.c_int64()
        self._chk(self.lib.elmk_water_balance(self.ctx, float(dt), _p(mms), C.byref(nbad), C.byref(first)), "water_balance")
        return mms, nbad.value, first.value

    def water_balance_read(self, which, col0=0, n=None):
        """Row `which` (hydrology.WB_BEGWB .. hydrology.WB_TOTSOILICE) of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("water_balance_read", which, col0, n, self.ncols, clamp=True)

    def water_balance_rows(self):
        """Every row of the feature: float64 [WB_NROWS, ncols], the `wb` of hydrology.water_balance_end."""
        return np.stack([self.water_balance_read(w) for w in range(WB_NROWS)])

    def water_balance_clear(self):
        """Free the rows, the scratch and the run's ring rows.  Refused while history entries over the rows exist."""
        self._chk(self.lib.elmk_water_balance_clear(self.ctx), "water_balance_clear")

    def run_water_balance(self):
        """Of the last run (synchronises), if it carried RUN_WATER_BALANCE: (min, max, sum) [nsteps, 3, 3] of ERRH2O, QRUNOFF, ENDWB,
        nbad [nsteps], first bad column [nsteps]; empty arrays otherwise."""
        m = max(getattr(self, "_run_max", 0), 1)
        mms, nb, fb = np.zeros((m, 3, 3)), np.zeros(m, np.int64), np.zeros(m, np.int64)
        n = self._chk(self.lib.elmk_run_water_balance(self.ctx, _p(mms), _p(nb), _p(fb)), "run_water_balance")
        return mms[:n].copy(), nb[:n].copy(), fb[:n].copy()

    def active_layer_update(self, rollover=0):
        """ELM's alt_calc for every column from the current t_soisno: one launch, stream-ordered, no sync.  rollover: ALT_ROLL_* bits
        (active_layer.rollover gives the run's rule).  Needs the column geography."""
        self._chk(self.lib.elmk_active_layer_update(self.ctx, int(rollover)), "active_layer_update")

    def active_layer_read(self, which, col0=0, n=None):
        """Row ALT_ALT, ALT_ALTMAX or ALT_ALTMAX_LASTYEAR of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("active_layer_read", which, col0, n, self.ncols)

    def active_layer_clear(self):
        """Free the three rows (the index fields keep their values)."""
        self._chk(self.lib.elmk_active_layer_clear(self.ctx), "active_layer_clear")

    # -- soil hydrology (include/elmk.h: elmk_soil_hydrology_enable ...; elmkernels_amd/hydrology.py restates the stage) -----------
    def soil_hydrology_enable(self):
        """Allocate the rows of the feature (fp64, zero-filled).  Refused when already enabled or while the stream is captured."""
        self._chk(self.lib.elmk_soil_hydrology_enable(self.ctx), "soil_hydrology_enable")

    def soil_hydrology_set_params(self, hksat, wtfact, h2osfc_thresh, k_wet, rsub_top_max):
        """The parameter rows: hksat [10, ncols] (hydrology.hksat_from_texture) and four [ncols] rows (scalars are broadcast)."""
        hk = np.ascontiguousarray(hksat, dtype=np.float64)
        if hk.shape != (HYD_NLAYER, self.ncols):
            raise ValueError(f"soil_hydrology_set_params: hksat must be [{HYD_NLAYER}, {self.ncols}]")
        one = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.ncols,))) for v in
               (wtfact, h2osfc_thresh, k_wet, rsub_top_max)]
        self._chk(self.lib.elmk_soil_hydrology_set_params(self.ctx, _p(hk), *(_p(v) for v in one)), "soil_hydrology_set_params")

    def soil_hydrology_init(self, zwt=None, wa=None):
        """ZWT and WA from [ncols] each; None: ELM's cold start (wa = 4000 mm, zwt = hydrology.cold_start_zwt).  Synchronises."""
        self._init_rows("soil_hydrology_init", (zwt, wa), "columns")

    def soil_hydrology(self, dt):
        """The stage for every column: one launch, stream-ordered, no sync.  Call after advance_physics."""
        self._chk(self.lib.elmk_soil_hydrology(self.ctx, float(dt)), "soil_hydrology")

    def soil_hydrology_read(self, which, col0=0, n=None):
        """Row `which` (hydrology.ZWT .. hydrology.FSAT) of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("soil_hydrology_read", which, col0, n, self.ncols)

    def soil_hydrology_rows(self):
        """Every row of the feature: float64 [HYD_NROWS, ncols], the `rows` of hydrology.step."""
        return np.stack([self.soil_hydrology_read(w) for w in range(HYD_NROWS)])

    def soil_hydrology_clear(self):
        """Free the rows, the frost-table extension's too (the state fields keep their values)."""
        self._chk(self.lib.elmk_soil_hydrology_clear(self.ctx), "soil_hydrology_clear")

    def soil_hydrology_frost_enable(self, q_perch_max):
        """The frost-table extension (include/elmk.h, F'): allocate its rows and upload q_perch_max [ncols] (hydrology.q_perch_max; a
        scalar is broadcast).  From here on soil_hydrology and run(..., soil_hydrology=True) drain perched water above frozen layers.
        Refused without the hydrology, when already enabled or while the stream is captured."""
        if q_perch_max is None:
            q = None
        else:
            q = np.ascontiguousarray(np.broadcast_to(np.asarray(q_perch_max, dtype=np.float64), (self.ncols,)))
        self._chk(self.lib.elmk_soil_hydrology_frost_enable(self.ctx, None if q is None else _p(q)), "soil_hydrology_frost_enable")

    def soil_hydrology_frost_read(self, which, col0=0, n=None):
        """Row `which` (hydrology.Q_PERCH_MAX .. hydrology.QFLX_DRAIN_PERCHED) of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("soil_hydrology_frost_read", which, col0, n, self.ncols)

    def soil_hydrology_frost_rows(self):
        """Every row of the extension: float64 [HYDF_NROWS, ncols], the `frost` of hydrology.step."""
        return np.stack([self.soil_hydrology_frost_read(w) for w in range(HYDF_NROWS)])

    def soil_hydrology_frost_clear(self):
        """Free the extension's rows only: the stage is the plain one again."""
        self._chk(self.lib.elmk_soil_hydrology_frost_clear(self.ctx), "soil_hydrology_frost_clear")

    # -- hillslope lateral flow (include/elmk.h: elmk_hillslope_enable ...; hydrology.hillslope_head / hillslope_flow / step(lat=)) ------
    def hillslope_enable(self, down, dist, width, area, elev, k_aniso):
        """Order the columns along hillslopes (include/elmk.h, L1 - L3): down int32 [ncols] (>= 0 the downhill column, -1 the stream,
        -2 on no hillslope), dist, width, area, elev float64 [ncols] (scalars are broadcast), k_aniso the ratio of horizontal to vertical
        conductivity.  From here on soil_hydrology and run(..., RUN_HYDROLOGY) pass groundwater downhill.  Refused without the hydrology,
        when already on, for a refusal of hydrology.hillslope_check, with the frost table or the floodplain infiltration on."""
        d = None if down is None else np.ascontiguousarray(down, dtype=np.int32).reshape(-1)
        if d is not None and d.size != self.ncols:
            raise ValueError(f"hillslope_enable: {d.size} values of down for {self.ncols} columns")
        a = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.ncols,)))
             for v in (dist, width, area, elev)]
        self._chk(self.lib.elmk_hillslope_enable(self.ctx, None if d is None else _p(d), *(None if v is None else _p(v) for v in a),
                                                 float(k_aniso)), "hillslope_enable")

    def hillslope_read(self, which, col0=0, n=None):
        """Row `which` (HS_HEAD .. HS_QSTREAM) of columns [col0, col0 + n): float64 [n].  Synchronises."""
        return self._read_row("hillslope_read", which, col0, n, self.ncols)

    def hillslope_rows(self):
        """Every row of the extension: float64 [HS_NROWS, ncols], the hs_out of hydrology.step(lat=)."""
        return np.stack([self.hillslope_read(w) for w in range(HS_NROWS)])

    def hillslope_budget(self):
        """float64 [1]: the sum of QSTREAM, m3/s (hydrology.hillslope_budget).  Synchronises."""
        sums = np.zeros(1)
        self._chk(self.lib.elmk_hillslope_budget(self.ctx, _p(sums)), "hillslope_budget")
        return sums

    def hillslope_clear(self):
        """Free the extension: the stage drains every column by its own baseflow again."""
        self._chk(self.lib.elmk_hillslope_clear(self.ctx), "hillslope_clear")

    # -- aerosol deposition (include/elmk.h: elmk_aerosol_reserve ...; elmkernels_amd/aerosol.py restates the kernel) ----------
    def aerosol_reserve(self, ncells=None, idx=None, w=None):
        """The device series of the eleven deposition streams x 12 months x ncells (fp64, zero-filled) and the map of the aerosol
        grid: idx int32 [npts, ncols] (-1 = padding, never in row 0) and w float64 [npts, ncols] (regrid.nearest_map,
        regrid.bilinear_map), or neither for per-column series (ncells = ncols).  Replaces an earlier reservation; the run reservation
        and the forcing grid stay."""
        if (idx is None) != (w is None):
            raise ValueError("idx and w: both or neither")
        if idx is None:
            ncells = self.ncols if ncells is None else int(ncells)
            self._chk(self.lib.elmk_aerosol_reserve(self.ctx, ncells, 0, None, None), "aerosol_reserve")
        else:
            npts, idx, w = self._ell_args(idx, w)
            if ncells is None:
                raise ValueError("aerosol_reserve: ncells of the aerosol grid is needed with a map")
            self._chk(self.lib.elmk_aerosol_reserve(self.ctx, int(ncells), npts, _p(idx), _p(w)), "aerosol_reserve")
        self.aerosol_ncells = int(ncells)

    def aerosol_upload(self, name, month0, records):
        """Months [month0, month0 + nmonths) of one stream ("aer_bcphi" .. "aer_dst4_2", or without the prefix) from records
        [nmonths, ncells] (or [ncells] for one month).  Waits for a run or deposition in flight that reads them."""
        a = np.ascontiguousarray(records, dtype=np.float64)
        if a.ndim == 1:
            a = a[None, :]
        nc = getattr(self, "aerosol_ncells", None)
        if nc is not None and a.shape[1] != nc:
            raise ValueError(f"{name}: {a.shape[1]} cell values per month, the series has {nc}")
        fid = self.fields[name if name in self.fields else "aer_" + name][0] if isinstance(name, str) else int(name)
        self._chk(self.lib.elmk_aerosol_upload(self.ctx, fid, int(month0), a.shape[0], _p(a)), f"aerosol_upload({name})")

    def aerosol_deposition(self, month1, month2, wt1, wt2):
        """aer_* of every column = wt1 * (month1 remapped) + wt2 * (month2 remapped), one launch, stream-ordered, no sync."""
        self._chk(self.lib.elmk_aerosol_deposition(self.ctx, int(month1), int(month2), float(wt1), float(wt2)), "aerosol_deposition")

    def aerosol_clear(self):
        """Free the aerosol series and map (aer_* keep their values)."""
        self._chk(self.lib.elmk_aerosol_clear(self.ctx), "aerosol_clear")
        self.aerosol_ncells = None

    # -- multi-step runs (include/elmk.h: elmk_run ...) ---------------------------------------------
    def run_reserve(self, forcing_slots, max_steps):
        """Device series of `forcing_slots` forcing records and 12 months, and step tables / diagnostics rings of `max_steps` rows."""
        self._chk(self.lib.elmk_run_reserve(self.ctx, int(forcing_slots), int(max_steps)), "run_reserve")
        self._run_max = int(max_steps)

    def series_upload(self, name, slot0, records, col0=0):
        """Records [slot0, slot0 + nslots) of one series field (SERIES_FORCING: forcing slots, SERIES_PHENOLOGY: months 0..11) from
        records [nslots, n] (record-major), columns [col0, col0 + n).  Waits for a run in flight only if it reads those records.
        With a forcing grid set at run_reserve, SERIES_FORCING records are cell records: [nslots, n] cells [col0, col0 + n)."""
        a = np.ascontiguousarray(records, dtype=np.float64)
        if a.ndim == 1:
            a = a[None, :]
        self._chk(self.lib.elmk_series_upload(self.ctx, self.fields[name][0], int(slot0), a.shape[0], _p(a),
                                              int(col0), a.shape[1]), f"series_upload({name})")

    def run(self, dt, steps, flags=0):
        """elmk_run: len(steps) model steps on the device, steps a RUN_STEP_DTYPE array; stream-ordered, no synchronisation."""
        a = np.ascontiguousarray(steps, dtype=RUN_STEP_DTYPE)
        self._chk(self.lib.elmk_run(self.ctx, float(dt), _p(a), int(a.size), int(flags)), "run")

    def run_diagnostics(self):
        """Of the last run (synchronises): conservation (min, max, sum) [nsteps, 8, 3], flag OR [nsteps], first fatal column [nsteps]."""
        m = max(getattr(self, "_run_max", 0), 1)
        mms, fo, fb = np.zeros((m, 8, 3)), np.zeros(m, np.uint32), np.zeros(m, np.int64)
        n = self._chk(self.lib.elmk_run_diagnostics(self.ctx, _p(mms), _p(fo), _p(fb)), "run_diagnostics")
        return mms[:n].copy(), fo[:n].copy(), fb[:n].copy()

    # -- shortwave (include/elmk.h: elmk_set_shortwave_mode ...) -------------------------------------
    def set_shortwave_mode(self, mode, forc_dt=0.0):
        """"reference" (the default, the reference's ProcessFSDS) or "coszen" (ELM's cos(zenith) factor over forcing records that are
        means over forc_dt seconds; needs a column geography).  A change forgets every record time."""
        code = SW_MODES[mode] if isinstance(mode, str) else int(mode)
        self._chk(self.lib.elmk_set_shortwave_mode(self.ctx, code, float(forc_dt)), "set_shortwave_mode")

    def set_forcing_record_time(self, rec_decday):
        """COSZEN, stepwise: the start of the record in level 0 of atm_* (decimal_doy + 1.0); enqueues the czf kernel."""
        self._chk(self.lib.elmk_set_forcing_record_time(self.ctx, float(rec_decday)), "set_forcing_record_time")

    def series_record_times(self, slot0, rec_decday):
        """COSZEN, runs: the record start (decimal_doy + 1.0) of forcing slots slot0 .. slot0 + len(rec_decday) - 1."""
        a = np.ascontiguousarray(rec_decday, dtype=np.float64).reshape(-1)
        self._chk(self.lib.elmk_series_record_times(self.ctx, int(slot0), a.size, _p(a)), "series_record_times")

    def forcing_cosz(self):
        """czf [ncols]: the forcing interval's mean cos(zenith) of the last record time or COSZEN run step (synchronises)."""
        out = np.empty(self.ncols)
        self._chk(self.lib.elmk_download_forcing_cosz(self.ctx, _p(out)), "forcing_cosz")
        return out

    # -- downscaling (include/elmk.h: elmk_set_downscaling ...) ---------------------------------------
    def _cols(self, a, what):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        if a.size != self.ncols:
            raise ValueError(f"{what} must be [{self.ncols}]")
        return a

    def set_column_elevation(self, topo_col, topo_forc=None):
        """The column elevations and the forcing's surface height as each column sees it (m, [ncols] each); topo_forc None sets only
        the columns' (the forcing's then comes from set_forcing_elevation_gridded)."""
        hc = self._cols(topo_col, "topo_col")
        hf = None if topo_forc is None else self._cols(topo_forc, "topo_forc")
        self._chk(self.lib.elmk_set_column_elevation(self.ctx, _p(hc), None if hf is None else _p(hf)), "set_column_elevation")

    def set_forcing_elevation_gridded(self, cells):
        """The forcing's surface height from its grid's cells [ncells], remapped through the forcing map (regrid.apply_map)."""
        a = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1)
        if getattr(self, "grid_ncells", None) is not None and a.size != self.grid_ncells:
            raise ValueError(f"{a.size} cell values, the grid has {self.grid_ncells}")
        self._chk(self.lib.elmk_set_forcing_elevation_gridded(self.ctx, _p(a)), "set_forcing_elevation_gridded")

    def set_downscaling(self, mode, lapse=LAPSE, lapse_lw=LAPSE_LW, lw_limit=LW_LIMIT):
        """"off" (the default) or "topo": forcing adjusted from the forcing's surface height to each column's elevation."""
        code = DS_MODES[mode] if isinstance(mode, str) else int(mode)
        self._chk(self.lib.elmk_set_downscaling(self.ctx, code, float(lapse), float(lapse_lw), float(lw_limit)), "set_downscaling")

    def set_downscaling_groups(self, ptr, col, w):
        """Longwave renormalisation groups, CSR by gridcell (regrid.owner_map builds one): ptr int64 [ngroups + 1], col int32 [nnz],
        w float64 [nnz]; a column in at most one group, weights finite and >= 0."""
        ngroups, ptr, col, w = _csr_args(ptr, col, w, "ngroups")
        self._chk(self.lib.elmk_set_downscaling_groups(self.ctx, ngroups, _p(ptr), _p(col), _p(w)), "set_downscaling_groups")

    def clear_downscaling_groups(self):
        self._chk(self.lib.elmk_clear_downscaling_groups(self.ctx), "clear_downscaling_groups")

    def column_elevation(self):
        """(topo_col, topo_forc) as held on the device (synchronises)."""
        hc, hf = np.empty(self.ncols), np.empty(self.ncols)
        self._chk(self.lib.elmk_download_column_elevation(self.ctx, _p(hc), _p(hf)), "column_elevation")
        return hc, hf

    # -- forcing on a coarser grid (include/elmk.h: elmk_set_forcing_grid ...) -----------------------
    def set_forcing_grid(self, idx, w, ncells):
        """The per-column remap map (elmkernels_amd/regrid.py): idx int32 [npts, ncols] (-1 = padding, never in row 0), w float64
        [npts, ncols], ncells source cells.  Releases the run reservation (run_reserve again before run)."""
        npts, idx, w = self._ell_args(idx, w)
        self._chk(self.lib.elmk_set_forcing_grid(self.ctx, int(ncells), npts, _p(idx), _p(w)), "set_forcing_grid")
        self.grid_ncells = int(ncells)

    def clear_forcing_grid(self):
        """Per-column forcing again; releases the run reservation."""
        self._chk(self.lib.elmk_clear_forcing_grid(self.ctx), "clear_forcing_grid")
        self.grid_ncells = None

    def upload_gridded(self, name, cells, level=0):
        """One level of an fp64 field from cell values [ncells], remapped to every column on the device."""
        a = np.ascontiguousarray(cells, dtype=np.float64).reshape(-1)
        if getattr(self, "grid_ncells", None) is not None and a.size != self.grid_ncells:
            raise ValueError(f"{name}: {a.size} cell values, the grid has {self.grid_ncells}")
        self._chk(self.lib.elmk_upload_gridded(self.ctx, self.fields[name][0], int(level), _p(a)), f"upload_gridded({name})")

    # -- output grid (include/elmk.h: elmk_set_output_grid ...) ----------------------------------------
    def set_output_grid(self, ptr, col, w, fill=np.nan):
        """The CSR aggregation map by output cell (elmkernels_amd/regrid.py: owner_map, from_sparse_cells): ptr int64 [ncells + 1],
        col int32 [nnz] (columns), w float64 [nnz]; a cell without terms reads `fill`.  Refused while gridded history entries exist."""
        ncells, ptr, col, w = _csr_args(ptr, col, w, "ncells")
        self._chk(self.lib.elmk_set_output_grid(self.ctx, ncells, _p(ptr), _p(col), _p(w), float(fill)), "set_output_grid")
        self.output_ncells = ncells

    def clear_output_grid(self):
        """Forget the output map (refused while gridded history entries exist)."""
        self._chk(self.lib.elmk_clear_output_grid(self.ctx), "clear_output_grid")
        self.output_ncells = None

    def download_gridded(self, name, level=0):
        """One level of field `name` aggregated onto the output cells on the device: float64 [ncells]."""
        if self.output_ncells is None:
            raise L.ElmkError("download_gridded: no output grid (set_output_grid)")
        out = np.empty(self.output_ncells, dtype=np.float64)
        self._chk(self.lib.elmk_download_gridded(self.ctx, self.fields[name][0], int(level), _p(out)), f"download_gridded({name})")
        return out

    def gridded_history_add(self, tape, name, op):
        """As history_add, with the accumulators on the output cells: every accumulate folds the aggregate of each level.  Returns
        the entry id; history_read of it is cell-shaped."""
        fid = self.fields[name][0] if isinstance(name, str) else int(name)
        code = HIST_OPS[op] if isinstance(op, str) else int(op)
        entry = self._chk(self.lib.elmk_gridded_history_add(self.ctx, int(tape), fid, code), f"gridded_history_add({name})")
        nlev = C.c_int()
        self.lib.elmk_field_info(fid, C.byref(nlev), None)
        self._hist_nlev[entry] = nlev.value
        self._hist_cells.add(entry)
        return entry

    def gridded_history_add_row(self, tape, family, which, op):
        """As history_add_row, with the accumulator on the output cells (gridded_history_add)."""
        fam = ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        code = HIST_OPS[op] if isinstance(op, str) else int(op)
        entry = self._chk(self.lib.elmk_gridded_history_add_row(self.ctx, int(tape), fam, int(which), code),
                          f"gridded_history_add_row({family}, {which})")
        self._hist_nlev[entry] = 1
        self._hist_cells.add(entry)
        return entry

    def cell_history_add_row(self, tape, family, which, op):
        """As history_add over one fp64 cell row of the river stages: family "routing" (which = ROUTE_*: the rows routing_read takes
        at this moment) or "supply" (IRRSUP_*, while the river supply limit is on), or CELL_ROWS_*.  One level, accumulators over the
        routing's cells; no map and no fill - every cell is a sample, one without columns in the output grid's map included.
        history_read of it returns [ncells].  While the entry exists the clears that would free its row, and set_output_grid /
        clear_output_grid, are refused (history_clear first).  history.fold_cell_rows restates the fold."""
        fam = CELL_ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        code = HIST_OPS[op] if isinstance(op, str) else int(op)
        entry = self._chk(self.lib.elmk_cell_history_add_row(self.ctx, int(tape), fam, int(which), code),
                          f"cell_history_add_row({family}, {which})")
        self._hist_nlev[entry] = 1
        self._hist_cells.add(entry)  # (the routing's cells are the output grid's)
        return entry

    # -- point series (include/elmk.h "point series"; elmkernels_amd/points.py restates a record and the ring's order) ---------
    def points_set(self, kind, idx):
        """The list of `kind` ("columns" / "cells" or ELMK_POINTS_*): int64 indices in any order, duplicates allowed, at most 4096;
        copied.  Every index is checked against ncols, or the output grid's ncells.  Only before the first record or after
        points_reset."""
        k = {"columns": 0, "cells": 1}[kind] if isinstance(kind, str) else int(kind)
        a = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        self._chk(self.lib.elmk_points_set(self.ctx, k, a.size, _p(a)), f"points_set({kind})")
        self._points_n[k] = a.size

    def _points_added(self, entry, k):
        self._points_kind[entry] = k
        return entry

    def points_add_field(self, name, level=0):
        """One level of a state field at the columns list; returns the entry id."""
        fid = self.fields[name][0] if isinstance(name, str) else int(name)
        return self._points_added(self._chk(self.lib.elmk_points_add_field(self.ctx, fid, int(level)), f"points_add_field({name}, {level})"), 0)

    def points_add_row(self, family, which):
        """One feature row (history_add_row's families) at the columns list; returns the entry id."""
        fam = ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        return self._points_added(self._chk(self.lib.elmk_points_add_row(self.ctx, fam, int(which)), f"points_add_row({family}, {which})"), 0)

    def points_add_cell_row(self, family, which):
        """One cell row of the river stages (cell_history_add_row's families) at the cells list; returns the entry id."""
        fam = CELL_ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        return self._points_added(self._chk(self.lib.elmk_points_add_cell_row(self.ctx, fam, int(which)), f"points_add_cell_row({family}, {which})"), 1)

    def points_add_gridded_field(self, name, level=0):
        """One level of a state field aggregated through the output grid's map at the cells list; returns the entry id."""
        fid = self.fields[name][0] if isinstance(name, str) else int(name)
        return self._points_added(self._chk(self.lib.elmk_points_add_gridded_field(self.ctx, fid, int(level)),
                                            f"points_add_gridded_field({name}, {level})"), 1)

    def points_add_gridded_row(self, family, which):
        """One feature row aggregated through the output grid's map at the cells list; returns the entry id."""
        fam = ROW_FAMILIES[family] if isinstance(family, str) else int(family)
        return self._points_added(self._chk(self.lib.elmk_points_add_gridded_row(self.ctx, fam, int(which)),
                                            f"points_add_gridded_row({family}, {which})"), 1)

    def points_reserve(self, max_records):
        """The ring: max_records records of the present entries, device-resident."""
        self._chk(self.lib.elmk_points_reserve(self.ctx, int(max_records)), "points_reserve")

    def points_record(self, stamp):
        """One record of every (entry, point) pair with time stamp `stamp`: one launch, stream-ordered, no synchronisation."""
        self._chk(self.lib.elmk_points_record(self.ctx, float(stamp)), "points_record")

    def points_set_run(self, on=True):
        """While on, every step of run() records once after the history stage, stamped with the step's decday."""
        self._chk(self.lib.elmk_points_set_run(self.ctx, 1 if on else 0), "points_set_run")

    def points_count(self):
        """(total, held): the records since the last reset and how many of them the ring still holds.  Does not synchronise."""
        t, h = C.c_int64(), C.c_int64()
        self._chk(self.lib.elmk_points_count(self.ctx, C.byref(t), C.byref(h)), "points_count")
        return t.value, h.value

    def points_read(self, entry, rec0=0, nrec=None):
        """float64 [nrec, npoints] of one entry: held records rec0 .. rec0 + nrec - 1, oldest first (nrec None: to the newest).
        Synchronises."""
        if nrec is None:
            nrec = self.points_count()[1] - int(rec0)
        out = np.empty((max(int(nrec), 0), self._points_n[self._points_kind.get(int(entry), 0)]), dtype=np.float64)
        self._chk(self.lib.elmk_points_read(self.ctx, int(entry), _p(out), int(rec0), int(nrec)), f"points_read({entry})")
        return out

    def points_stamps(self, rec0=0, nrec=None):
        """float64 [nrec]: the stamps of the same records.  Synchronises."""
        if nrec is None:
            nrec = self.points_count()[1] - int(rec0)
        out = np.empty(max(int(nrec), 0), dtype=np.float64)
        self._chk(self.lib.elmk_points_stamps(self.ctx, _p(out), int(rec0), int(nrec)), "points_stamps")
        return out

    def points_reset(self):
        """total back to 0 and the run's recording off; entries, lists and the reservation stay."""
        self._chk(self.lib.elmk_points_reset(self.ctx), "points_reset")

    def points_clear(self):
        """Free the part: entries, lists, reservation."""
        self._chk(self.lib.elmk_points_clear(self.ctx), "points_clear")
        self._points_n, self._points_kind = [0, 0], {}

    # -- restart images (include/elmk.h "restart"; elmkernels_amd/restart.py reads and rewrites them on the host) -------------
    def field_class(self, name):
        """CLASS_PROGNOSTIC, CLASS_SURFACE, CLASS_FORCING or CLASS_DIAGNOSTIC (include/elmk_restart.def)."""
        return field_class(name)

    def restart_size(self):
        n = C.c_int64()
        self._chk(self.lib.elmk_restart_size(self.ctx, C.byref(n)), "restart_size")
        return n.value

    def restart_save(self, gcol0=0):
        """The image of this context's columns, global columns [gcol0, gcol0 + ncols): np.ndarray of uint8."""
        img = np.empty(self.restart_size(), np.uint8)
        self._chk(self.lib.elmk_restart_save(self.ctx, int(gcol0), img.ctypes.data, img.size), "restart_save")
        return img

    def restart_load(self, image, gcol0=0):
        """Verify the whole image, then load its fields, history accumulators and tape counts and the accumulated fields' values and
        step counts; the history and accumulator entries must have been registered as when it was saved."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        self._chk(self.lib.elmk_restart_load(self.ctx, int(gcol0), img.ctypes.data, img.size), "restart_load")

    def math_eval(self, fn, x, y=None):
        """elmk_math.h on the device: fn in MATH_FNS; returns fn(x), x / y or pow(x, y)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.float64)
            assert y.shape == x.shape
            yp = _p(y)
        self._chk(self.lib.elmk_math_eval(self.ctx, MATH_FNS.index(fn), _p(x), yp, _p(out), x.size), "math_eval")
        return out


MATH_FNS = ["exp", "log", "log10", "atan", "sqrt", "tanh", "cos", "erf", "acos", "expm1", "div", "pow", "sin"]
WRAPPER_NAMES = ["frac_wet", "albedo_snicar", "canopy_hydrology", "surface_radiation", "canopy_temperature",
                 "bareground_fluxes", "canopy_fluxes", "soil_temperature", "surface_fluxes", "snow_hydrology", "advance_physics"]
KERNEL_NAMES = [
    "frac_wet", "albedo_snicar", "canopy_hydrology", "surface_radiation", "canopy_temperature",
    "bareground_fluxes", "canopy_fluxes",
]
# launch groups of elmk_timestep7_fused (include/elmk.h: elmk_profile_timestep7_fused)
KERNEL_NAMES_FUSED = ["prep_frac_wet", "albedo_snicar", "fused_stream", "bareground_list", "canopy_iterate"]


# ---- the L3 wrappers, named as in driver/kokkos/*_kokkos.hh ------------------------------------------
def kokkos_frac_wet(S):
    S._chk(S.lib.elmk_frac_wet(S.ctx), "frac_wet")


def kokkos_albedo_snicar(S):
    S._chk(S.lib.elmk_albedo_snicar(S.ctx), "albedo_snicar")


def kokkos_canopy_hydrology(S, dt):
    S._chk(S.lib.elmk_canopy_hydrology(S.ctx, float(dt)), "canopy_hydrology")


def kokkos_surface_radiation(S):
    S._chk(S.lib.elmk_surface_radiation(S.ctx), "surface_radiation")


def kokkos_canopy_temperature(S):
    S._chk(S.lib.elmk_canopy_temperature(S.ctx), "canopy_temperature")


def kokkos_bareground_fluxes(S):
    S._chk(S.lib.elmk_bareground_fluxes(S.ctx), "bareground_fluxes")


def kokkos_canopy_fluxes(S, dt):
    S._chk(S.lib.elmk_canopy_fluxes(S.ctx, float(dt)), "canopy_fluxes")


def _opt(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def canopy_fluxes_given(S, dt, forc_rho=None, forc_po2=None, forc_pco2=None):
    """L2-level canopy_fluxes: forcing-derived scalars handed in (test/test_CanFlux.cc) instead of derived by the wrapper."""
    a = [_opt(x) for x in (forc_rho, forc_po2, forc_pco2)]
    assert all(x is None or x.shape == (S.ncols,) for x in a)
    S._chk(S.lib.elmk_canopy_fluxes_given(S.ctx, float(dt), *[None if x is None else _p(x) for x in a]), "canopy_fluxes_given")


def bareground_fluxes_given(S, forc_rho):
    """L2-level bareground_fluxes with ELM's own air density (test/test_BGFlux.cc)."""
    a = _opt(forc_rho)
    assert a.shape == (S.ncols,)
    S._chk(S.lib.elmk_bareground_fluxes_given(S.ctx, _p(a)), "bareground_fluxes_given")


def kokkos_soil_temperature(S, dt):
    """Next in ELMInterface::advance after the seven (elm_kokkos_interface.cc:310; soil_temperature_kokkos.cc:6-278)."""
    S._chk(S.lib.elmk_soil_temperature(S.ctx, float(dt)), "soil_temperature")


def kokkos_snow_hydrology(S, dt):
    """snow_hydrology_kokkos.cc:23-188 (between soil_temperature and surface_fluxes in ELMInterface::advance, :313)."""
    S._chk(S.lib.elmk_snow_hydrology(S.ctx, float(dt)), "snow_hydrology")


def get_forcing(S, wt1, wt2, qbot_is_rh=False):
    """ELM::get_forcing (atm_forcing_kokkos.cc:47-75); wt1, wt2: [8] weights of TBOT, PBOT, QBOT|RH, FLDS, FSDS, PREC, WIND, ZBOT."""
    w1 = np.ascontiguousarray(wt1, dtype=np.float64)
    w2 = np.ascontiguousarray(wt2, dtype=np.float64)
    assert w1.shape == (8,) and w2.shape == (8,)
    S._chk(S.lib.elmk_get_forcing(S.ctx, _p(w1), _p(w2), int(bool(qbot_is_rh))), "get_forcing")


def compute_phenology(S, wt1, wt2):
    """ComputePhenology (phenology_physics_impl.hh:22-69) as update_phenology runs it (phenology_kokkos.cc:59-62)."""
    S._chk(S.lib.elmk_phenology(S.ctx, float(wt1), float(wt2)), "phenology")


def forcing_time_weights(days_since_record, forc_dt):
    """AtmDataManager::forcing_time_weights (atm_data_impl.hh:191-199): (wt1, wt2) for a model time `days_since_record`
    days after the forcing record t_idx, records `forc_dt` days apart."""
    e = days_since_record / forc_dt
    assert 0.0 <= e <= 1.0
    return 1.0 - e, e


def initialize_kokkos_elm(S):
    """The per-column init functions of ELM::initialize_kokkos_elm (initialize_elm_kokkos.cc:373-428) - cold-start state from
    topography, snow depth, soil texture and PFT; the file reads of that function stay with the caller."""
    S._chk(S.lib.elmk_initialize_state(S.ctx), "initialize_state")


def kokkos_init_timestep(S):
    """The per-column kernel of kokkos_init_timestep (init_timestep_kokkos.cc:55-75)."""
    S._chk(S.lib.elmk_init_timestep(S.ctx), "init_timestep")


def kokkos_surface_fluxes(S, dt):
    """surface_fluxes_kokkos.cc:5-107 (follows soil_temperature in ELMInterface::advance)."""
    S._chk(S.lib.elmk_surface_fluxes(S.ctx, float(dt)), "surface_fluxes")


CONSERVATION_NAMES = ("dtend_column_h2o", "errh2o", "errh2osno", "dwb", "errsol", "errlon", "errseb", "netrad")


def kokkos_evaluate_conservation(S, dt, per_column=False):
    """conserved_quantity_kokkos.cc:8-81 -> min_max_sum [8, 3] (rows: CONSERVATION_NAMES) and, if asked, the
    per-column values [ncols, 8]."""
    mms = np.zeros((8, 3))
    cols = np.zeros((8, S.ncols)) if per_column else None
    S._chk(S.lib.elmk_evaluate_conservation(S.ctx, float(dt), _p(mms), _p(cols) if per_column else None), "evaluate_conservation")
    return (mms, np.ascontiguousarray(cols.T)) if per_column else mms


def timestep7_fused(S, dt):
    """The same seven calls with the streaming wrappers between albedo and the leaf-temperature iteration fused into one
    pass per column (elmk_timestep7_fused); bit-identical results."""
    S._chk(S.lib.elmk_timestep7_fused(S.ctx, float(dt)), "timestep7_fused")


def advance_physics(S, dt):
    """Every per-column call of ELMInterface::advance after kokkos_init_timestep, in its order
    (elm_kokkos_interface.cc:289-316): the seven wrappers (fused), soil_temperature, snow_hydrology, surface_fluxes - one
    call (elmk_advance_physics), one HIP graph launch per step with set_graph(True).  Same bits as the ten calls."""
    S._chk(S.lib.elmk_advance_physics(S.ctx, float(dt)), "advance_physics")


def timestep7(S, dt):
    """The seven calls of ELMInterface::advance (driver/kokkos/elm_kokkos_interface.cc:289-307), in order."""
    S._chk(S.lib.elmk_timestep7(S.ctx, float(dt)), "timestep7")


class ELMInterface:
    """Python mirror of the reference's driver class ELM::ELMInterface (driver/kokkos/elm_kokkos_interface.hh:11-28,
    elm_kokkos_interface.cc:38-358) above the C ABI, the counterpart of include/elmk_interface.hpp: same member names, same call
    order in advance(), same PrimaryVars members (src/data/elm_state.h:17-48).  File reads and date arithmetic stay with
    the caller, who uploads fields / forcing records and passes the interpolation weights."""

    PRIMARY_VARS = ("snl", "snow_depth", "frac_sno", "int_snow", "snw_rds", "h2osoi_liq", "h2osoi_ice", "h2osoi_vol", "h2ocan",
                    "h2osno", "h2osfc", "t_soisno", "t_grnd", "t_h2osfc", "t_h2osfc_bef", "nrad", "dz", "zsoi", "zisoi")

    def __init__(self, ncols, device=0):
        self.S = ELMState(ncols, device=device)
        self.conservation = None

    def setup(self, land, scalars, pft, snicar, soilcolor, snow_age_tables, init_params=None, graph=True):
        """ELMInterface::setup (elm_kokkos_interface.cc:58-267) minus the file reads."""
        S = self.S
        S.set_land(**land)
        S.set_scalars(**scalars)
        S.set_pft(pft)
        S.set_snicar(snicar)
        S.set_soilcolor(*soilcolor)
        S.set_snow_age_tables(snow_age_tables)
        if init_params is not None:
            S.set_init_params(*init_params)
        S.set_graph(bool(graph))

    def initialize(self):
        """The per-column part of ELM::initialize_kokkos_elm (initialize_elm_kokkos.cc:373-428), after the uploads."""
        initialize_kokkos_elm(self.S)

    def advance(self, dt_seconds, forc_wt1, forc_wt2, month_wt1, month_wt2, qbot_is_rh=False):
        """ELMInterface::advance (elm_kokkos_interface.cc:269-322); returns False like the reference."""
        S = self.S
        compute_phenology(S, month_wt1, month_wt2)
        get_forcing(S, forc_wt1, forc_wt2, qbot_is_rh)
        kokkos_init_timestep(S)
        advance_physics(S, dt_seconds)
        self.conservation = kokkos_evaluate_conservation(S, dt_seconds)
        flags, col = S.error_summary()
        if flags & 0xC7FF:  # ELMK_ERR_FATAL_MASK
            raise RuntimeError(f"ELM physics error flags {flags:#x}, first at column {col}")
        return False

    def run(self, dt_seconds, steps, accumulate_history=False, qbot_is_rh=False, update_accum=False, update_aerosol=False,
            update_active_layer=False, soil_hydrology=False, water_balance=False, irrigation=False, routing=False):
        """ELMInterface::advance for every row of steps (RUN_STEP_DTYPE) in one call (elmk_run; needs S.run_reserve and the series
        uploaded); self.conservation = the last step's triples, self.run_conservation = all of them.  update_accum: every step updates
        the accumulated fields registered on self.S (ELM's UpdateAccVars: after the physics, before the history).  update_aerosol: every
        step interpolates aer_* from the aerosol series of self.S (S.aerosol_reserve / aerosol_upload) over the step's month bracket,
        between the forcing and init_timestep.  update_active_layer: every step runs ELM's alt_calc after the physics (S.active_layer_enable),
        with the annual rollover on the steps that start at 00:00 of 1 January / 1 July.  water_balance: every step closes the water budget
        (S.water_balance_enable; with soil_hydrology); self.run_water_balance = S.run_water_balance() of the run.  irrigation: every step
        applies and checks irrigation between the seven wrappers and soil_temperature (S.irrigation_enable; dt a whole number of seconds).  routing: every step
        routes the step's runoff after the water balance (S.routing_enable; with water_balance).  Raises after the run if a step raised a fatal flag, naming the first such step and column."""
        S = self.S
        flags = (RUN_HISTORY if accumulate_history else 0) | (RUN_QBOT_IS_RH if qbot_is_rh else 0) | (RUN_ACCUM if update_accum else 0)
        flags |= (RUN_AEROSOL if update_aerosol else 0) | (RUN_ALT if update_active_layer else 0)
        flags |= RUN_HYDROLOGY if soil_hydrology else 0  # the soil hydrology stage after surface_fluxes (S.soil_hydrology_enable)
        flags |= RUN_WATER_BALANCE if water_balance else 0
        flags |= RUN_IRRIGATION if irrigation else 0
        flags |= RUN_ROUTING if routing else 0
        S.run(dt_seconds, steps, flags)
        if water_balance:
            self.run_water_balance = S.run_water_balance()
        mms, fo, fb = S.run_diagnostics()
        self.run_conservation = mms
        self.conservation = mms[-1]
        bad = np.nonzero(fo & 0xC7FF)[0]  # ELMK_ERR_FATAL_MASK
        if bad.size:
            s = int(bad[0])
            raise RuntimeError(f"ELM physics error flags {int(fo[s]):#x} in step {s} of the run, first at column {int(fb[s])}")
        return False

    def set_shortwave_mode(self, mode, forc_dt=0.0):
        """ELMState.set_shortwave_mode: "coszen" spreads interval-mean FSDS records over their steps (after the geography is set)."""
        self.S.set_shortwave_mode(mode, forc_dt)

    def set_forcing_record_time(self, rec_decday):
        self.S.set_forcing_record_time(rec_decday)

    def series_record_times(self, slot0, rec_decday):
        self.S.series_record_times(slot0, rec_decday)

    def set_column_elevation(self, topo_col, topo_forc=None):
        """ELMState.set_column_elevation: each column's elevation and the forcing's surface height as it sees it (m)."""
        self.S.set_column_elevation(topo_col, topo_forc)

    def set_forcing_elevation_gridded(self, cells):
        self.S.set_forcing_elevation_gridded(cells)

    def set_downscaling(self, mode, lapse=LAPSE, lapse_lw=LAPSE_LW, lw_limit=LW_LIMIT):
        """ELMState.set_downscaling: "topo" adjusts every step's forcing to the column elevations (after they are set)."""
        self.S.set_downscaling(mode, lapse, lapse_lw, lw_limit)

    def set_downscaling_groups(self, ptr, col, w):
        self.S.set_downscaling_groups(ptr, col, w)

    def clear_downscaling_groups(self):
        self.S.clear_downscaling_groups()

    def set_forcing_grid(self, idx, w, ncells):
        """Forcing on the data set's own grid (ELMState.set_forcing_grid): then upload_gridded() per record, or reserve a run and
        upload cell records with S.series_upload."""
        self.S.set_forcing_grid(idx, w, ncells)

    def clear_forcing_grid(self):
        self.S.clear_forcing_grid()

    def upload_gridded(self, name, cells, level=0):
        self.S.upload_gridded(name, cells, level)

    def accumulate_history(self):
        """Fold this step's state into the history tapes registered on self.S (ELMState.history_add): call after advance()."""
        self.S.history_accumulate()

    def update_aerosol(self, month1, month2, wt1, wt2):
        """aer_* from the aerosol series of self.S (ELMState.aerosol_deposition): call before advance(), with the month bracket that
        feeds advance()'s month_wt1 / month_wt2 (the reference's hook, init_timestep_kokkos.cc:48-49)."""
        self.S.aerosol_deposition(month1, month2, wt1, wt2)

    def update_active_layer(self, rollover=0):
        """ELM's alt_calc on self.S (ELMState.active_layer_update): call after advance(), before update_accum()."""
        self.S.active_layer_update(rollover)

    def update_accum(self):
        """Update the accumulated fields registered on self.S (ELMState.accum_add): call after advance(), before accumulate_history()."""
        self.S.accum_update()

    def restart_save(self, gcol0=0):
        """The restart image of the columns (ELMState.restart_save)."""
        return self.S.restart_save(gcol0)

    def restart_load(self, image, gcol0=0):
        """After setup(), the geography and maps and the same history entries: load an image instead of initialize()."""
        self.S.restart_load(image, gcol0)

    def restart_size(self):
        return self.S.restart_size()

    def field_class(self, name):
        return self.S.field_class(name)

    def getPrimaryVars(self):
        """ELMInterface::getPrimaryVars / copyPrimaryVars (:324-356): the PrimaryVars members as host arrays."""
        return {k: self.S[k] for k in self.PRIMARY_VARS}

    def close(self):
        self.S.close()
