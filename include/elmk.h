/*
 * elmk.h - C ABI of libelmk: MI355X-native (gfx950 / HIP) per-gridcell land-surface physics.
 *
 * Drop-in boundary for the reference's L3 dispatch layer.  The reference exposes, per physics group, a
 * C++ free function  void ELM::kokkos_<physics>(ELMStateType& S [, const double& dt])  declared in
 * driver/kokkos/<physics>_kokkos.hh and called only from ELMInterface::advance
 * (driver/kokkos/elm_kokkos_interface.cc:287-319).  Each elmk_<physics>() below replaces one of them;
 * the ELMState object becomes an opaque context that owns the same named per-column arrays on the GPU.
 *
 *   reference (file:line)                                             replacement
 *   ---------------------------------------------------------------   ---------------------------------
 *   ELMState(ncols, ...)            src/data/elm_state.h:184-192      elmk_create
 *   ~ELMState                                                         elmk_destroy
 *   S.<field> Views                 src/data/elm_state.h:53-180       elmk_upload / elmk_download /
 *                                                                     elmk_device_ptr  (ids: elmk_fields.def)
 *   S.Land                          src/data/land_data.h:36-44        elmk_set_land
 *   S.dewmx/oldfflag/dayl/max_dayl  src/data/elm_state.h:221-224      elmk_set_scalars
 *   kokkos_init_timestep's coszen / dayl / max_dayl (per column)
 *                                   init_timestep_kokkos.cc:26-34     elmk_set_column_geography, elmk_solar_geometry
 *   S.pft_data (PFTData)            src/data/pft_data.h:20-31,35-90   elmk_set_pft
 *   S.albsat / S.albdry             src/data/elm_state.h:82           elmk_set_soilcolor
 *   S.snicar_data (SnicarData)      src/data/snicar_data.h:29-71      elmk_set_snicar
 *   kokkos_frac_wet(S)              canopy_hydrology_kokkos.hh:10     elmk_frac_wet
 *   kokkos_albedo_snicar(S)         albedo_kokkos.hh                  elmk_albedo_snicar
 *   kokkos_canopy_hydrology(S,dt)   canopy_hydrology_kokkos.hh:7      elmk_canopy_hydrology
 *   kokkos_surface_radiation(S)     surface_radiation_kokkos.hh       elmk_surface_radiation
 *   kokkos_canopy_temperature(S)    canopy_temperature_kokkos.hh      elmk_canopy_temperature
 *   kokkos_bareground_fluxes(S)     bareground_fluxes_kokkos.hh       elmk_bareground_fluxes
 *   kokkos_canopy_fluxes(S,dt)      canopy_fluxes_kokkos.hh           elmk_canopy_fluxes
 *   advance(): the 7 calls in order elm_kokkos_interface.cc:289-307   elmk_timestep7, elmk_timestep7_fused
 *   advance(): all per-column calls elm_kokkos_interface.cc:289-316   elmk_advance_physics
 *   get_forcing(S, dt, date)        atm_forcing_kokkos.cc:47-75       elmk_get_forcing
 *   update_phenology: ComputePhenology  phenology_kokkos.cc:59-62     elmk_phenology
 *   kokkos_init_timestep's kernel   init_timestep_kokkos.cc:55-75     elmk_init_timestep
 *   initialize_kokkos_elm's lambda  initialize_elm_kokkos.cc:373-428  elmk_initialize_state
 *   kokkos_soil_temperature(S,dt)   soil_temperature_kokkos.hh        elmk_soil_temperature
 *   kokkos_snow_hydrology(S,dt,t)   snow_hydrology_kokkos.hh          elmk_snow_hydrology
 *   S.snw_rds_table (SnwRdsTable)   src/data/snicar_data.h:75-84      elmk_set_snow_age_tables
 *   kokkos_surface_fluxes(S,dt)     surface_fluxes_kokkos.hh          elmk_surface_fluxes
 *   kokkos_evaluate_conservation    conserved_quantity_kokkos.hh      elmk_evaluate_conservation
 *   (ELM's history tapes: time averages, extremes, last values)       elmk_history_add / _accumulate / _read
 *   (ELM's accumulMod: T10, the running means behind photosynthesis)  elmk_accum_add / _init / _update / _read
 *   kokkos_driver.cc:54-85 time loop                                  elmk_run (elmk_run_reserve, elmk_series_upload)
 *   AtmDataManager::data(ntimes, ncells) on the data set's own grid   elmk_set_forcing_grid, elmk_upload_gridded,
 *     (src/data/atm_data.h:168-172; ELM's coupler maps it to land)     elmk_series_upload of cell records
 *   ELM's c2g: columns averaged onto grid cells by area for history  elmk_set_output_grid, elmk_download_gridded,
 *     and for the fluxes a coupled run returns to the atmosphere       elmk_gridded_history_add
 *   throw / assert inside physics   (list: SURVEY.md section 5)       per-column flag word, elmk_error_summary
 *
 * Conventions
 *   - every function returns 0 on success, a negative elmk_status on API misuse / HIP failure
 *     (elmk_last_error gives the text); physics never fails a call - reference throw/assert sites raise
 *     bits in a per-column flag word instead (ELMK_ERR_*), readable with elmk_error_summary or by
 *     downloading ELMK_FIELD_err_flags.
 *   - plain pointers and sizes only; host buffers are caller-owned and touched only inside
 *     upload/download/set_*; the context owns all device memory (allocated once in elmk_create).
 *   - kernel entry points enqueue on the context's HIP stream and return; elmk_sync / elmk_download wait.
 *   - one context per GPU; different contexts may be driven from different host threads.
 *   - there is no CPU fallback: without a usable HIP device elmk_create fails with ELMK_E_NO_DEVICE.
 */
#ifndef ELMK_H
#define ELMK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct elmk_ctx elmk_ctx;

/* dimensions (src/data/elm_constants.h:84-98) */
enum {
  ELMK_NLEVSNO = 5,
  ELMK_NLEVGRND = 15,
  ELMK_NLEVTOT = 20,
  ELMK_NUMRAD = 2,
  ELMK_NLEVCAN = 1,
  ELMK_NUMRAD_SNW = 5,
  ELMK_SNO_NBR_AER = 8,
  ELMK_MXPFT = 25,
  ELMK_NSOILCOL = 20,
  ELMK_MIE_N = 1471,
  ELMK_PSN_NPARAM = 27, /* members of ELM::PFTDataPSN, in declaration order (pft_data.h:20-24) */
  ELMK_ALB_NPARAM = 9   /* rhol[2] rhos[2] taul[2] taus[2] xl (pft_data.h:27-31) */
};

typedef enum {
  ELMK_OK = 0,
  ELMK_E_INVALID = -1,   /* bad argument (null pointer, unknown field, range) */
  ELMK_E_NO_DEVICE = -2, /* no HIP device / device id out of range */
  ELMK_E_HIP = -3,       /* a HIP runtime call failed */
  ELMK_E_NOMEM = -4
} elmk_status;

/* element types of fields */
typedef enum { ELMK_F64 = 0, ELMK_I32 = 1, ELMK_U8 = 2, ELMK_U32 = 3 } elmk_dtype;

/* host-side layouts accepted by upload/download */
typedef enum {
  ELMK_LAYOUT_COL_MAJOR = 0, /* reference layout: [column][level], level fastest (ELM::Array / LayoutRight) */
  ELMK_LAYOUT_SOA = 1        /* [level][column], column fastest, dense (stride = ncols of the transfer) */
} elmk_layout;

/* field ids: ELMK_FIELD_<name>, generated from elmk_fields.def; err_flags is appended */
typedef enum {
#define ELMK_FIELD(name, T, nlev) ELMK_FIELD_##name,
#include "elmk_fields.def"
#undef ELMK_FIELD
  ELMK_FIELD_err_flags,
  ELMK_NUM_FIELDS
} elmk_field;

/* per-column error flags, one bit per reference throw / assert site */
enum {
  ELMK_ERR_SURFRAD_LAYER_SUM = 1u << 0, /* surface_radiation_impl.hh:173 assert */
  ELMK_ERR_CANFLX_FORC_HGT = 1u << 1,   /* canopy_fluxes_impl.hh:178 assert(zldis >= 0) */
  ELMK_ERR_PSN_NEG_GS = 1u << 2,        /* photosynthesis_impl.hh:232 */
  ELMK_ERR_PSN_QUADRATIC = 1u << 3,     /* photosynthesis_impl.hh:289 */
  ELMK_ERR_PSN_BRENT_BRACKET = 1u << 4, /* photosynthesis_impl.hh:439 */
  ELMK_ERR_ALB_CANOPY_LAYERS = 1u << 5, /* surface_albedo_impl.hh:270 */
  ELMK_ERR_SNICAR_RDS = 1u << 6,        /* snow_snicar_impl.hh:76 */
  ELMK_ERR_SNICAR_FLAG = 1u << 7,       /* snow_snicar_impl.hh:99 */
  ELMK_ERR_SNICAR_NEG_ABS = 1u << 8,    /* snow_snicar_impl.hh:618 */
  ELMK_ERR_SNICAR_ENERGY = 1u << 9,     /* snow_snicar_impl.hh:658 */
  ELMK_ERR_SNICAR_ALBEDO = 1u << 10,    /* snow_snicar_impl.hh:664 */
  ELMK_WARN_PSN_BALL_BERRY = 1u << 11,  /* photosynthesis_impl.hh:240 (std::cout warning, not fatal) */
  /* elmk_snow_hydrology.  Two places where the reference reads outside an array, so that its own result is undefined; the
   * column continues with the documented choice and the flag records that it was taken (not fatal):
   *   snow_hydrology_impl.hh:388  snow_water reads vol_ice[i+i] (meant i+1) of a 5-element array; i <= 2 is in bounds and is
   *                               reproduced literally, for i = 3 (index 6) vol_ice[i+1] is used;
   *   snow_hydrology_impl.hh:871-885  combine_layers' shift loop copies element top-1 into top; with five snow layers that
   *                               is element -1 of the level arrays: 0.0 is used (the element ends up above the pack and
   *                               is reset by prune_snow_layers / the aerosol update / snow_aging).
   * and the path's two throw sites (fatal): */
  ELMK_WARN_SNOW_WATER_OOB = 1u << 12,
  ELMK_WARN_SNOW_COMBINE_OOB = 1u << 13,
  ELMK_ERR_SNOW_DIVIDE_RDS = 1u << 14,  /* snow_hydrology_impl.hh:1032, :1109, :1187, :1253 radius outside the Mie table */
  ELMK_ERR_SNOW_AGE_DRFRESH = 1u << 15  /* snow_hydrology_impl.hh:152 dr_fresh < 0 */
};
#define ELMK_ERR_FATAL_MASK 0xC7FFu

/* SNICAR lookup tables, names and extents of ELM::SnicarData (src/data/snicar_data.h:39-69); all row-major */
typedef struct {
  const double *ss_alb_oc1, *asm_prm_oc1, *ext_cff_mss_oc1;             /* [5] */
  const double *ss_alb_oc2, *asm_prm_oc2, *ext_cff_mss_oc2;             /* [5] */
  const double *ss_alb_dst1, *asm_prm_dst1, *ext_cff_mss_dst1;          /* [5] */
  const double *ss_alb_dst2, *asm_prm_dst2, *ext_cff_mss_dst2;          /* [5] */
  const double *ss_alb_dst3, *asm_prm_dst3, *ext_cff_mss_dst3;          /* [5] */
  const double *ss_alb_dst4, *asm_prm_dst4, *ext_cff_mss_dst4;          /* [5] */
  const double *ss_alb_snw_drc, *asm_prm_snw_drc, *ext_cff_mss_snw_drc; /* [5][1471] */
  const double *ss_alb_snw_dfs, *asm_prm_snw_dfs, *ext_cff_mss_snw_dfs; /* [5][1471] */
  const double *ss_alb_bc1, *asm_prm_bc1, *ext_cff_mss_bc1;             /* [10][5] */
  const double *ss_alb_bc2, *asm_prm_bc2, *ext_cff_mss_bc2;             /* [10][5] */
  const double *bcenh;                                                  /* [8][10][5] */
} elmk_snicar_tables;

/* one perturbation rule of elmk_tile_columns */
typedef struct {
  int32_t field;  /* elmk_field */
  int32_t mode;   /* 0: v *= (1 + amp*u), 1: v += amp*u,  u ~ U(-1,1) from a counter-based hash */
  double amp;
} elmk_perturb;

/* ---- lifetime ------------------------------------------------------------------------------- */
int elmk_create(int64_t ncols, int device_id, elmk_ctx **out);
int elmk_destroy(elmk_ctx *ctx);
const char *elmk_last_error(const elmk_ctx *ctx); /* ctx may be NULL: error of the last failed create */
int elmk_set_stream(elmk_ctx *ctx, void *hip_stream); /* hipStream_t; NULL restores the context's own stream */
int elmk_sync(elmk_ctx *ctx);
/* on != 0: elmk_timestep7 captures its ~22 kernel launches (and the side-stream fork / join inside albedo_snicar) once as
 * a HIP graph and replays it on every call with the same dt and stream.  Same kernels, same order, same results; what
 * it removes is per-launch host latency, which is all there is to a step of a few thousand columns. */
int elmk_set_graph(elmk_ctx *ctx, int on);
/* Launch options of a context (no effect on results, bit for bit).
 *   ELMK_OPT_CF_HALF_WORKGROUPS  value != 0: the leaf-temperature iteration of kokkos_canopy_fluxes (k_cf_iterate) runs in 256-thread
 *     workgroups, one per compute unit - half the registers and 68 KB of a CU's LDS stay free, so the kernels of ANOTHER context's
 *     stream are resident on the same CUs and use the memory pipeline this fp64-bound kernel leaves idle.  For a driver that steps two
 *     (or more) blocks of columns as separate contexts on separate streams; on its
 *     own the kernel is 1.5 x slower in this shape, which is why it is an option.
 *   ELMK_OPT_ALB_STAGED  value != 0: kokkos_albedo_snicar (and elmk_timestep7's) runs SNICAR of the one-layer snow packs and the final
 *     stage as launches of their own (k_alb_snicar<1>, k_alb_final) that meet through device memory, instead of k_alb_tile, which does
 *     both for a tile of 256 columns in one workgroup and is the default.  The structure an A/B or a test compares k_alb_tile with. */
enum { ELMK_OPT_CF_HALF_WORKGROUPS = 1, ELMK_OPT_ALB_STAGED = 2 };
/* Not a launch option: ELMK_OPT_RESTART_CELLS, value != 0: the restart image of a context with the runoff routing enabled carries the
 * river stages' state (image format, version 6, under "restart"); off, the default, every image is byte for byte what it was.  Refused
 * while the stream is being captured. */
enum { ELMK_OPT_RESTART_CELLS = 3 };
int elmk_set_option(elmk_ctx *ctx, int option, int value);
int64_t elmk_ncols(const elmk_ctx *ctx);
int64_t elmk_level_stride(const elmk_ctx *ctx); /* elements between consecutive levels of a device field */
int64_t elmk_device_bytes(const elmk_ctx *ctx);

/* ---- schema --------------------------------------------------------------------------------- */
int elmk_num_fields(void);
const char *elmk_field_name(int field);
int elmk_field_id(const char *name); /* -1 if unknown */
int elmk_field_info(int field, int *nlev, int *dtype);
/* bytes the device keeps per element of an fp64 field: 8 in the product (libelmk.so); 4 in libelmk_f32.so, the report-only
 * build of BASELINE config 5 ("fp32 state": every fp64 field stored as fp32, all arithmetic fp64, widen on load / round on
 * store).  The ABI is the same in both: uploads and downloads speak double. */
int elmk_state_real_bytes(void);

/* ---- data movement -------------------------------------------------------------------------- */
/* columns [col0, col0+n) of one field; host buffer holds n*nlev elements in the given layout */
int elmk_upload(elmk_ctx *ctx, int field, const void *host, int64_t col0, int64_t n, int layout);
int elmk_download(elmk_ctx *ctx, int field, void *host, int64_t col0, int64_t n, int layout);
int elmk_fill(elmk_ctx *ctx, int field, double value); /* every level of every column */
void *elmk_device_ptr(elmk_ctx *ctx, int field);      /* SoA base: element (lev, col) at [lev*stride + col] */
/* replicate columns [0, nbase) into [nbase, ncols) - column c takes column c % nbase - applying the given
 * perturbations (synthetic-workload generator for the benchmark) */
int elmk_tile_columns(elmk_ctx *ctx, int64_t nbase, uint64_t seed, int nrules, const elmk_perturb *rules);
/* Keep a device-side copy of the listed fields as they are now (replaces any earlier snapshot), and copy
 * them back later (a streaming copy kernel on the context's stream).  A driver uses this for
 * what the rest of the model would do between two calls of the hot path - e.g. the reference resets the
 * forcing heights every step (atm_physics_impl.hh:197-203) and other components move t_veg; the benchmark
 * uses it so that every timed step starts from the same, unconverged canopy state. */
int elmk_snapshot_fields(elmk_ctx *ctx, const int *fields, int nfields);
int elmk_restore_fields(elmk_ctx *ctx);

/* ---- parameters ----------------------------------------------------------------------------- */
int elmk_set_land(elmk_ctx *ctx, int ltype, int ctype, int vtype, int urbpoi, int lakpoi);
int elmk_set_scalars(elmk_ctx *ctx, double dewmx, int oldfflag, double dayl, double max_dayl);
/* psn[25][27], alb[25][9], z0mr[25], displar[25] */
int elmk_set_pft(elmk_ctx *ctx, const double *psn, const double *alb, const double *z0mr, const double *displar);
int elmk_set_soilcolor(elmk_ctx *ctx, const double *albsat /*[20][2]*/, const double *albdry /*[20][2]*/);
int elmk_set_snicar(elmk_ctx *ctx, const elmk_snicar_tables *t);
/* SnwRdsTable (src/data/snicar_data.h:75-84): the snow-aging best-fit parameters snowage_tau [hour], snowage_kappa and
 * snowage_drdt0 [um/hour], each [11][31][8] = [temperature][temperature gradient][density] index, row-major */
int elmk_set_snow_age_tables(elmk_ctx *ctx, const double *tau, const double *kappa, const double *drdt0);

/* ---- per-column solar geometry ----------------------------------------------------------------
 * kokkos_init_timestep computes ONE step-averaged cos(zenith), day length and maximum day length for the whole domain on the
 * host, at S.lat_r / S.lon_r (init_timestep_kokkos.cc:26-34: "only one value currently"), and elmk_interface.hpp's
 * ELMInterface::set_solar_geometry does the same.  These entries do it for every column at its own location, on the device, with
 * the reference's bits for that column:
 *   elmk_set_column_geography  lat_r, lon_r: [ncols] radians, |lat_r| <= pi/2 + 10 eps (day_length.cc:22), finite lon_r; copied,
 *                              not retained.  The time-invariant terms (tan / sin / cos of the latitude, max_daylength) are
 *                              computed here once, with the host libm.  Setting a geography alone changes nothing.
 *   elmk_solar_geometry        for every column c: coszen[c] = average_cosz(lat_c, lon_c, dt, decday), the day length
 *                              daylength(lat_c, declination_angle_sin(doy + 1)) and max_daylength(lat_c) - decday =
 *                              decimal_doy(date) + 1.0 and doy = date.doy, the arguments ELMInterface::set_solar_geometry takes.
 *                              Enqueued on the context's stream.  From the first call on, the context is in per-column mode:
 *                              canopy_fluxes (every path to it - elmk_canopy_fluxes, _given, elmk_timestep7(_fused),
 *                              elmk_advance_physics, their graphs, ELMK_OPT_CF_HALF_WORKGROUPS) takes the day-length factor of
 *                              photosynthesis from each column's own dayl / max_dayl instead of elmk_set_scalars' two scalars;
 *                              a column gives the bits a scalar-mode context with elmk_set_scalars(dayl_c, max_dayl_c) gives.
 *                              ELMK_E_INVALID without a geography.
 *   elmk_download_day_length   [ncols] each (either may be NULL) of the last elmk_solar_geometry; synchronises.
 *   elmk_clear_column_geography  back to scalar mode (elmk_set_scalars' dayl / max_dayl); the geography is forgotten, coszen keeps
 *                              its values.
 * A multi-rank driver passes each rank its own slice of the grid (elmkernels_amd/decomp.py). */
int elmk_set_column_geography(elmk_ctx *ctx, const double *lat_r, const double *lon_r);
int elmk_solar_geometry(elmk_ctx *ctx, double dt_seconds, double decday, int doy);
int elmk_download_day_length(elmk_ctx *ctx, double *dayl, double *max_dayl);
int elmk_clear_column_geography(elmk_ctx *ctx);

/* ---- history --------------------------------------------------------------------------------
 * Output averaged over time without a download per step (ELM's history tapes): a driver registers fields once, folds the
 * current state into device-resident accumulators with one launch per step, and downloads only at the end of an output interval.
 *   elmk_history_add         register every level of `field` on `tape` (0 .. ELMK_HIST_MAX_TAPES-1) with `op`; returns the entry
 *                            id (>= 0, in order of registration) or a negative ELMK_E_* code.  Refused: an unknown field, op or
 *                            tape, a full table (ELMK_HIST_MAX_ENTRIES over all tapes), a tape that has accumulated samples since
 *                            its last reset, a stream that is being captured.  Allocates nlev x level-stride fp64 on the device.
 *   elmk_history_accumulate  fold the current value of every registered field of every tape into its accumulator and count one
 *                            sample for each tape that has entries: ONE kernel launch on the context's stream, no host memory, no
 *                            synchronisation - a caller may capture it into a graph of its own.  Nothing without entries.  A
 *                            captured graph holds the entry table of the moment of capture: capture again after add / clear.
 *   elmk_history_reset       stream-ordered and capturable: the tape's accumulators back to their initial values, its count to 0
 *   elmk_history_count       the tape's sample count, kept on the device (a replayed graph counts every replay); synchronises
 *   elmk_history_read        the entry's result as doubles, [nlev] per column, columns [col0, col0+n), layout as elmk_download;
 *                            ELMK_E_INVALID while its tape holds 0 samples; synchronises
 *   elmk_history_clear       drop every entry of every tape and free its buffers; counts to 0
 * Semantics, bit for bit: a sample is the stored value widened to fp64 (F64 as stored - fp32 widened in libelmk_f32.so -, I32 /
 * U8 / U32 exactly); accumulators are fp64.  SUM / AVG: -0.0 after a reset, then acc = acc + v in step order; SUM reads acc, AVG
 * reads acc / (double)count (one correctly rounded division when read, not a running mean).  MAX: -inf after a reset, then
 * acc = (v > acc || v != v) ? v : acc, so a NaN sticks; MIN the mirror image from +inf.  INST: the last sample.
 * Accumulating writes no state field and no physics scratch and changes no other call, graph or launch shape. */
enum { ELMK_HIST_AVG = 0, ELMK_HIST_SUM = 1, ELMK_HIST_MAX = 2, ELMK_HIST_MIN = 3, ELMK_HIST_INST = 4 };
#define ELMK_HIST_MAX_TAPES 4
#define ELMK_HIST_MAX_ENTRIES 64 /* per context, over all tapes */
int elmk_history_add(elmk_ctx *ctx, int tape, int field, int op);
int elmk_history_accumulate(elmk_ctx *ctx);
int elmk_history_reset(elmk_ctx *ctx, int tape);
int elmk_history_count(elmk_ctx *ctx, int tape, int64_t *nsamples);
int elmk_history_read(elmk_ctx *ctx, int entry, double *host, int64_t col0, int64_t n, int layout);
int elmk_history_clear(elmk_ctx *ctx);

/* ---- multi-step runs ------------------------------------------------------------------------
 * The reference's driver time loop (kokkos_driver.cc:54-85: one ELMInterface::advance per step) as one call: the forcing and
 * phenology records stay on the device as series, the host sends the schedule of N steps in one copy, and nothing in the run
 * synchronises with the host.
 *   elmk_run_reserve     allocates everything a run needs (counted in elmk_device_bytes): the forcing series (atm_tbot .. atm_wind x
 *                        forcing_slots records), the phenology series (mlai, msai, mhtop, mhbot x 12 months), two step tables of
 *                        max_steps rows and two diagnostics rings.  Series start at 0.  Calling it again waits for the runs in
 *                        flight and re-reserves (the series contents are lost).  forcing_slots >= 2, max_steps >= 1.
 *   elmk_series_upload   records [slot0, slot0 + nslots) of one series field - ELMK_FIELD_atm_tbot .. ELMK_FIELD_atm_wind (slots
 *                        0 .. forcing_slots-1) or ELMK_FIELD_mlai .. ELMK_FIELD_mhbot (slots = months 0 .. 11) - columns [col0, col0+n)
 *                        from host[nslots][n] (record-major: AtmDataManager::data(ntimes, ncells)); stored at state precision
 *                        (rounded as elmk_upload rounds in libelmk_f32.so).  The copy runs on an internal stream, so it overlaps a
 *                        run in flight; it first waits for any enqueued, unfinished run that reads one of the slots it writes.
 *                        Returns when the copy is done.
 *   elmk_run             for each step s, the bits of the calls
 *                          elmk_solar_geometry(dt, decday, doy); elmk_phenology(month_wt1, month_wt2) over months month1 / month2;
 *                          elmk_get_forcing(forc_wt1, forc_wt2, flags & ELMK_RUN_QBOT_IS_RH) over slots forc_slot / forc_slot + 1;
 *                          with ELMK_RUN_AEROSOL: elmk_aerosol_deposition(month1, month2, month_wt1, month_wt2) ("aerosol deposition");
 *                          elmk_init_timestep; elmk_advance_physics(dt) - with ELMK_RUN_IRRIGATION: its split form with
 *                          elmk_irrigation(dt, the step's time of day) before elmk_soil_temperature ("irrigation");
 *                          with ELMK_RUN_HYDROLOGY: elmk_soil_hydrology(dt) ("soil hydrology");
 *                          elmk_evaluate_conservation -> ring row s;
 *                          elmk_error_summary -> ring row s (flags sticky, as that call sees them after the step);
 *                          with ELMK_RUN_ROUTING: elmk_routing(dt) after the step's water balance ("runoff routing");
 *                          with ELMK_RUN_ALT: elmk_active_layer_update(the step's rollover) ("active layer thickness");
 *                          with ELMK_RUN_ACCUM: elmk_accum_update ("accumulated fields");
 *                          with ELMK_RUN_HISTORY: elmk_history_accumulate.
 *                        Stream-ordered, returns without synchronising; with elmk_set_graph one step is captured once (one chain of
 *                        nodes) and replayed nsteps times.  Enters per-column solar mode (as elmk_solar_geometry does).  Needs a
 *                        column geography, the snow-age tables and elmk_run_reserve.  ELMK_E_INVALID, before anything is enqueued,
 *                        for nsteps outside 1 .. max_steps, dt not finite and positive, a forc_slot outside 0 .. forcing_slots-2,
 *                        a month outside 0 .. 11, unknown flags, a stream being captured.  A run reads neither atm_* nor
 *                        mlai .. mhbot.  The step tables are double-buffered: run k+1 may be enqueued while run k executes;
 *                        enqueuing run k+2 waits until run k has finished.
 *   elmk_run_diagnostics synchronises, then copies the rows of the most recently enqueued run (any pointer may be NULL):
 *                        min_max_sum[nsteps][8][3] as elmk_evaluate_conservation (the same order of the sum, the same rule for
 *                        NaN and infinities: see there), flags_or[nsteps] and first_bad_col[nsteps] (-1: none) as elmk_error_summary.  Returns that run's nsteps (0 before the first run). */
typedef struct {
  double decday;                    /* decimal_doy(step start) + 1.0, as elmk_solar_geometry */
  int32_t doy;                      /* date.doy of the step start */
  int32_t forc_slot;                /* series slot of forcing record t_idx; slot forc_slot + 1 holds t_idx + 1 */
  double forc_wt1[8], forc_wt2[8];  /* as elmk_get_forcing (TBOT PBOT QBOT|RH FLDS FSDS PREC WIND ZBOT) */
  int32_t month1, month2;           /* phenology months 0 .. 11 bracketing the step (monthly_data.cc:29-37) */
  double month_wt1, month_wt2;      /* monthly_data.cc:56-62 */
} elmk_run_step;
enum { ELMK_RUN_QBOT_IS_RH = 1, ELMK_RUN_HISTORY = 2 };
#define ELMK_RUN_ACCUM 4 /* the third flag bit: every step updates the accumulated fields ("accumulated fields" below) */
#define ELMK_RUN_AEROSOL 8 /* the fourth flag bit: every step interpolates the aerosol deposition streams ("aerosol deposition" below) */
int elmk_run_reserve(elmk_ctx *ctx, int forcing_slots, int max_steps);
int elmk_series_upload(elmk_ctx *ctx, int field, int slot0, int nslots, const double *host, int64_t col0, int64_t n);
int elmk_run(elmk_ctx *ctx, double dt, const elmk_run_step *steps, int nsteps, int flags);
int elmk_run_diagnostics(elmk_ctx *ctx, double *min_max_sum, uint32_t *flags_or, int64_t *first_bad_col);

/* ---- forcing grid ----------------------------------------------------------------------------
 * Forcing on the data set's own grid (GSWP3 / CRUNCEP at 0.5 deg, ERA5 at 0.25 deg, an atmosphere's grid), remapped to the columns on
 * the device through a per-column map: the host sends ncells values per record instead of ncols.
 *   elmk_set_forcing_grid  the map, padded sparse rows in ELL form: up to npts source cells per column, idx[npts][ncols] and
 *                          w[npts][ncols] (SoA, column fastest; copied, not retained).  The value of column c of cell values a[ncells]
 *                          is, in this operation order and without contraction:
 *                            v = w[0][c] * a[idx[0][c]];  then for k = 1 .. npts-1:  if idx[k][c] >= 0:  v = v + w[k][c] * a[idx[k][c]]
 *                          idx = -1 is padding and is skipped, never multiplied by zero (-0.0 stays -0.0, a non-finite cell is not
 *                          read).  elmkernels_amd/regrid.py: apply_map is this operation on the host; nearest_map, bilinear_map and
 *                          from_sparse (a map file's row / col / S triplets) build maps, slice_map one rank's block.
 *                          ELMK_E_INVALID, nothing enqueued: npts outside 1 .. 8, ncells outside 1 .. 2^31-1, idx[0][c] outside
 *                          [0, ncells), idx[k][c] outside [-1, ncells) for k >= 1, a non-finite weight where idx >= 0, a stream being
 *                          captured.  Replaces an earlier map.
 *   elmk_clear_forcing_grid  forget the map: per-column forcing series again.
 *   Both wait for the runs in flight and release the run reservation as a new elmk_run_reserve does (series contents lost, the
 *   captured run step dropped); elmk_run refuses until the next elmk_run_reserve.
 *   elmk_upload_gridded    level `level` of any fp64 per-column field (atm_*, aer_*, mlai .. mhbot, surface data ...) from cells[ncells]:
 *                          the cells go to a staging buffer of the context, a kernel writes the remap of every column (stored at
 *                          state precision: rounded to fp32 in libelmk_f32.so, as elmk_upload rounds).  Synchronises as elmk_upload.
 *                          ELMK_E_INVALID without a map, for a field that is not fp64, a level out of range, a stream being captured.
 *   Run mode: elmk_run_reserve while a map is set sizes the seven forcing series slots x ncells (cell records; the phenology series
 *   stay per column); elmk_series_upload of atm_tbot .. atm_wind then takes cells [col0, col0 + n) of ncells, record-major
 *   host[nslots][n].  elmk_run remaps both records of every stream per step inside its forcing kernel.  For every column a run gives
 *   the bits of the same run over per-column series equal to the remap of each record (graph on and off).  In libelmk_f32.so the
 *   cell records are stored as fp32 and the remap is done in fp64 before the forcing arithmetic, so that holds bitwise only for maps
 *   with one term of weight 1.0 per column.
 *   Device memory (elmk_device_bytes): the map, npad x (4 + 8) bytes x elmk_level_stride with npad = npts rounded up to 1, 2, 4 or 8
 *   (padding rows), and ncells x 8 bytes of staging, each rounded up to 256 bytes. */
int elmk_set_forcing_grid(elmk_ctx *ctx, int64_t ncells, int npts, const int32_t *idx /*[npts][ncols]*/, const double *w /*[npts][ncols]*/);
int elmk_clear_forcing_grid(elmk_ctx *ctx);
int elmk_upload_gridded(elmk_ctx *ctx, int field, int level, const double *cells /*[ncells]*/);

/* ---- shortwave --------------------------------------------------------------------------------
 * ProcessFSDS (atm_physics_impl.hh:122-143) sets swndr = max(fsds * coszen * 0.5, 0) with a placeholder for ELM's cos(zenith) factor
 * (:126-130).  The FSDS records of the usual data sets (GSWP3: 3 h, CRUNCEP: 6 h) are means over the record's interval, so with the
 * placeholder a column receives the record times the step's mean cos(zenith) - less than the data set's sunlight, by an amount that
 * depends on the sun's height.  COSZEN mode applies ELM's factor, which spreads each record over the steps of its interval:
 *   cz  = coszen[c] (the step's mean: elmk_solar_geometry, elmk_run, or whatever the caller uploaded)
 *   czf = average_cosz(lat_c, lon_c, forc_dt, rec_decday) (incident_shortwave.cc:113-121), the mean over the record's interval;
 *         rec_decday = decimal_doy(start of record t_idx) + 1.0, the convention of elmk_solar_geometry's decday
 *   fac   = (cz > 0.001) ? min(cz / czf, 10.0) : 0.0       (min: the first argument wins ties and NaN)
 *   swndr = max(fsds * fac * 0.5, 0.0)                     (in this order, without contraction; the rest of get_forcing unchanged)
 * Both cosines are the reference's analytic means, so over one interval the steps' factors average to one (up to rounding) wherever
 * neither the 0.001 threshold nor the cap applies, and the record's energy is kept.  (ELM's offline driver averages cos(zenith)
 * sampled at the model steps instead; this is not imitated.)
 *   elmk_set_shortwave_mode     ELMK_SW_REFERENCE (the default: the reference's formula, bit for bit; forc_dt ignored) or
 *                               ELMK_SW_COSZEN with forc_dt_seconds the data set's record interval.  ELMK_E_INVALID: an unknown
 *                               mode; COSZEN without a column geography or with forc_dt not finite or outside (0, 86400 x 366]; a
 *                               stream being captured.  Waits for the runs in flight.  A change of mode or forc_dt forgets every
 *                               record time and drops the captured run step.  elmk_clear_column_geography puts a COSZEN context
 *                               back to REFERENCE.
 *   elmk_set_forcing_record_time  stepwise path: rec_decday of the record held in level 0 of atm_*.  Enqueues one kernel writing czf
 *                               of every column into a context buffer.  COSZEN mode only; in COSZEN mode elmk_get_forcing without a
 *                               record time is ELMK_E_INVALID.  An elmk_run overwrites the buffer: set the time again after it.
 *   elmk_series_record_times    run path: rec_decday of forcing slots [slot0, slot0 + nslots) (the record start of each slot).  COSZEN
 *                               mode and elmk_run_reserve needed; waits for a run that reads those slots, as elmk_series_upload.
 *                               elmk_run_reserve and elmk_set_forcing_grid / elmk_clear_forcing_grid forget the times; in COSZEN
 *                               mode elmk_run refuses, before anything is enqueued, any step whose forc_slot has no time.  Each step
 *                               of a COSZEN run computes czf beside coszen in its solar kernel.
 *   elmk_download_forcing_cosz  [ncols]: czf of the last record time or of the last run step; synchronises (tests, diagnostics).
 *                               ELMK_E_INVALID before either since the mode was set.
 * A context that never leaves REFERENCE mode runs the kernels, launch sequences and graphs it ran before and allocates nothing more.
 * COSZEN allocates ncols x 8 bytes (czf) on entering the mode and forcing_slots x 56 bytes (the record times) per reservation, both
 * counted in elmk_device_bytes.  The restart image does not change: mode and times are driver setup, like geography and maps.
 * libelmk_f32.so keeps czf and fac in fp64; its bits are report-only, as for the rest of that build. */
enum { ELMK_SW_REFERENCE = 0, ELMK_SW_COSZEN = 1 };
int elmk_set_shortwave_mode(elmk_ctx *ctx, int mode, double forc_dt_seconds);
int elmk_set_forcing_record_time(elmk_ctx *ctx, double rec_decday);
int elmk_series_record_times(elmk_ctx *ctx, int slot0, int nslots, const double *rec_decday /*[nslots]*/);
int elmk_download_forcing_cosz(elmk_ctx *ctx, double *czf /*[ncols]*/);

/* ---- downscaling -----------------------------------------------------------------------------
 * Forcing from a coarse grid carries the near-surface air at the forcing's surface height.  TOPO mode adjusts it to each column's own
 * elevation, as ELM's downscale_forcings (atm2lndMod) does.  With tg, pg, qg, Lg = tbot, pbot, qbot, lwrad exactly as get_forcing
 * computes them (clamps, the RH conversion and the FLDS fallback included), prec the PREC record ProcessPREC reads, hc the column's
 * elevation and hf the forcing's surface height as the column sees it (both in m), and RAIR, GRAV, CPAIR, TFRZ the constants of
 * elm_constants.h, the forcing kernel evaluates, left to right and without contraction (exp: the host libm's bits, qsat: the
 * reference's qsat_impl.hh; ZBOT = 30.0, ProcessZBOT's forc_hgt):
 *   dz   = hc - hf
 *   tc   = tg - lapse * dz
 *   Hbot = RAIR * 0.5 * (tg + tc) / GRAV
 *   pc   = pg * exp(-dz / Hbot)
 *   thc  = tg + (tc - tg) * exp((ZBOT / Hbot) * (RAIR / CPAIR))        (the forcing's potential temperature is tg)
 *   qc   = qg * (qs_c / qs_g)                                          (qs_g = qsat(tg, pg), qs_c = qsat(tc, pc): RH is kept)
 *   Lc   = max(min(Lg - lapse_lw * dz, Lg * (1.0 + lw_limit)), Lg * (1.0 - lw_limit))    (std::min / std::max)
 *   frac = min(1.0, max(0.0, (tc - TFRZ) * 0.5));  rain = frac * prec;  snow = (1.0 - frac) * prec
 * and writes forc_tbot = tc, forc_thbot = thc, forc_pbot = pc, forc_qbot = qc, forc_lwrad = Lc, forc_rain, forc_snow.  Shortwave,
 * wind and heights are unchanged (a COSZEN factor applies as it does without downscaling); forc_rho, po2, pco2 and vp are derived
 * from these fields downstream, as always.  hc == hf gives exactly the bits of OFF (exp(-0.0) = 1, qs / qs = 1, and the group
 * normalisation below is exactly 1): that is how a column is exempted.
 * Longwave groups (optional; ELM's downscale_longwave): a CSR map by gridcell, group g owns terms ptr[g] .. ptr[g+1]-1, each a column
 * col[p] with weight w[p].  Per group, with sums of one rounded product per term added in term order (as the output grid aggregates,
 * regrid.apply_aggregate): W = sum w, A = sum w * Lg, S = sum w * Lc; norm = (W == 0 || A == 0) ? 1.0 : (A / W) / (S / W); then
 * Lc = Lc * norm for every column of the group, so the group keeps its weighted mean longwave.  Columns of no group are not
 * renormalised.  Groups lie inside one context: a decomposition must keep a gridcell's columns on one rank (not checked).
 *   elmk_set_column_elevation   hc and hf, [ncols] each (copied).  topo_forc may be NULL: only hc is set (hf then comes from
 *                               elmk_set_forcing_elevation_gridded).  ELMK_E_INVALID for a non-finite value.
 *   elmk_set_forcing_elevation_gridded  hf from the forcing grid's surface height cells[ncells], remapped through the stored forcing
 *                               map exactly as elmk_upload_gridded remaps (regrid.apply_map), kept in fp64.  ELMK_E_INVALID without
 *                               a map or for a non-finite cell.  Clearing or replacing the map later leaves hf as it is.
 *   elmk_set_downscaling        ELMK_DS_OFF (the default) or ELMK_DS_TOPO, with lapse (K/m), lapse_lw (W m-2 per m) and lw_limit;
 *                               CLM5 / ELM's namelist values are 0.006, 0.032 and 0.5.  ELMK_E_INVALID: an unknown mode, TOPO before
 *                               both hc and hf are set, a non-finite parameter, lapse < 0, lapse_lw < 0, lw_limit outside [0, 1).
 *   elmk_set_downscaling_groups the groups (copied).  ELMK_E_INVALID as elmk_set_output_grid (ngroups outside 1 .. 2^31-1, ptr[0] != 0
 *                               or decreasing, nnz outside 0 .. 2^31-1, col outside [0, ncols)), and for a column in more than one
 *                               term, a weight not finite or negative.  Replaces earlier groups.
 *   elmk_clear_downscaling_groups  no groups.
 *   elmk_download_column_elevation  hc and / or hf (either pointer may be NULL); ELMK_E_INVALID for one not set.  Synchronises.
 * Every setter refuses while the stream is being captured, waits for the runs in flight and drops the captured run step; a refusal
 * enqueues nothing.  In TOPO mode elmk_get_forcing and every forcing kernel of elmk_run use the downscaling variant (per-column
 * series or a forcing grid, REFERENCE or COSZEN shortwave), followed by one renormalisation launch while groups are set; a run gives
 * the bits of the stepwise calls.  A context that never calls these runs the kernels, launch sequences and graphs it ran before and
 * allocates nothing more.  Device memory (elmk_device_bytes): 2 x 8 bytes x elmk_level_stride for the elevations (first setter), and
 * for groups 8 x (ngroups + 1) + 12 x nnz + 8 x ngroups + 8 x elmk_level_stride bytes (each region rounded up to 256).  The restart
 * image does not change: elevations, mode and groups are driver setup.  libelmk_f32.so keeps the elevations and the downscaling
 * arithmetic in fp64 and stores the results at state precision (report-only). */
enum { ELMK_DS_OFF = 0, ELMK_DS_TOPO = 1 };
int elmk_set_column_elevation(elmk_ctx *ctx, const double *topo_col /*[ncols]*/, const double *topo_forc /*[ncols] or NULL*/);
int elmk_set_forcing_elevation_gridded(elmk_ctx *ctx, const double *cells /*[ncells]*/);
int elmk_set_downscaling(elmk_ctx *ctx, int mode, double lapse, double lapse_lw, double lw_limit);
int elmk_set_downscaling_groups(elmk_ctx *ctx, int64_t ngroups, const int64_t *ptr /*[ngroups+1]*/, const int32_t *col /*[nnz]*/,
                                const double *w /*[nnz]*/);
int elmk_clear_downscaling_groups(elmk_ctx *ctx);
int elmk_download_column_elevation(elmk_ctx *ctx, double *topo_col /*[ncols] or NULL*/, double *topo_forc /*[ncols] or NULL*/);

/* ---- output grid -----------------------------------------------------------------------------
 * The other direction: columns aggregated onto an output grid on the device (ELM's c2g, area-weighted means of the columns of each
 * grid cell; the land -> atmosphere map of a coupled run), so a driver downloads ncells values per field level instead of ncols.
 *   elmk_set_output_grid   the map, CSR by output cell: nnz = ptr[ncells], cell i owns terms ptr[i] .. ptr[i+1]-1, each a column
 *                          col[p] and a weight w[p] (copied, not retained).  The value of cell i of a source row x (one level of a
 *                          field, each element widened to fp64 as history widens it) is, in this operation order and without
 *                          contraction:
 *                            ptr[i] == ptr[i+1]:  v = fill
 *                            otherwise:           v = w[p0] * x[col[p0]];  then for p = p0+1 .. p1-1:  v = v + w[p] * x[col[p]]
 *                          Weights are used as given (normalising them is the map builder's job).  elmkernels_amd/regrid.py:
 *                          apply_aggregate is this operation on the host; owner_map (area-weighted ownership) and from_sparse_cells
 *                          (a map file's row / col / S triplets) build maps, slice_output_map one rank's block.
 *                          ELMK_E_INVALID, nothing enqueued: ncells outside 1 .. 2^31-1, ptr[0] != 0 or ptr decreasing, nnz outside
 *                          0 .. 2^31-1, a col outside [0, ncols), a non-finite weight, a stream being captured, any gridded history
 *                          entry existing (elmk_history_clear first).  Replaces an earlier map.
 *   elmk_clear_output_grid forget the map; ELMK_E_INVALID while gridded history entries exist or the stream is being captured.
 *   The output grid is independent of the forcing grid and of the run reservation: setting or clearing it releases neither.
 *   elmk_download_gridded  level `level` of any field (F64 - stored as fp32 in libelmk_f32.so -, I32, U8, U32) aggregated into
 *                          cells[ncells] on the device; only those doubles are copied back.  Synchronises as elmk_download.
 *                          ELMK_E_INVALID without a map, for an unknown field, a level out of range, a stream being captured.
 *   elmk_gridded_history_add  as elmk_history_add (the same entry ids, table and limits, the same refusals, and without an output
 *                          grid), but the entry's accumulators live on the output cells, nlev x ncells: each elmk_history_accumulate
 *                          takes g = the aggregate of the current value of each level and folds it, acc = fold(op, acc, g), by the
 *                          rules of "history" (ELM's order: c2g, then the time fold).  A cell with no terms reads fill under every op.
 *                          elmk_history_read, _reset, _count and _clear work on gridded entries unchanged; for a gridded entry
 *                          elmk_history_read's col0, n index cells.  A tape with only gridded entries counts one sample per
 *                          accumulate.  With gridded entries elmk_history_accumulate stays one launch (the cell rows after the
 *                          column rows), stream-ordered, host-free and capturable, and elmk_run with ELMK_RUN_HISTORY folds them every
 *                          step; column entries give the same bits with or without gridded entries beside them.  Without gridded
 *                          entries nothing changes.
 *   Device memory (elmk_device_bytes): the map's ptr ((ncells + 1) x 8 bytes), col (nnz x 4) and w (nnz x 8), and each gridded
 *   entry's accumulators (nlev x ncells rounded up to 64 x 8 bytes), each rounded up to 256 bytes; elmk_clear_output_grid and
 *   elmk_history_clear return them. */
int elmk_set_output_grid(elmk_ctx *ctx, int64_t ncells, const int64_t *ptr /*[ncells+1]*/, const int32_t *col /*[nnz]*/,
                         const double *w /*[nnz]*/, double fill);
int elmk_clear_output_grid(elmk_ctx *ctx);
int elmk_download_gridded(elmk_ctx *ctx, int field, int level, double *cells /*[ncells]*/);
int elmk_gridded_history_add(elmk_ctx *ctx, int tape, int field, int op);

/* ---- accumulated fields -----------------------------------------------------------------------
 * ELM's accumulMod on the device: named fields accumulated over time from a source field, updated once per step after the physics
 * and before the history update (UpdateAccVars), and fed back into the state without a round trip through the host.  The one the hot
 * path reads is t10, the 10-day running mean of t_ref2m behind photosynthesis' acclimation terms (vcmaxse, jmaxse, jmax25top in
 * canopy_fluxes): no kernel of the step writes it, so without an entry it stays what was uploaded.
 * An entry has a source field (every level, any dtype, each sample widened to fp64 as history widens it), a kind, a period P >= 1 in
 * steps, an optional destination field, a value buffer val[nlev][level stride] in fp64 (in both builds) and a step count n kept on the
 * device: the updates folded in so far.  One update uses nstep = n + 1 and the sample v, per element, in this operation order and
 * without contraction (`/` is the correctly rounded fp64 division):
 *   ELMK_ACCUM_RUNMEAN   a = min(nstep, P);  val = ((double)(a - 1) * val + v) / (double)a     (as written also for a == 1)
 *   ELMK_ACCUM_TIMEAVG   if (nstep % P == 1 || P == 1) val = +0.0;  val = val + v;  if (nstep % P == 0) val = val / (double)P
 *   ELMK_ACCUM_RUNACCUM  if (rint(v) == -99999.0) val = +0.0;
 *                        else t = val + v;  t = t > 0.0 ? t : 0.0;  val = t < 99999.0 ? t : 99999.0
 * then n = n + 1.  The destination receives val at state precision (rounded to fp32 in libelmk_f32.so) on every update; for TIMEAVG
 * only on an update that completes a period, so that the field holds the last whole average.  elmkernels_amd/accum.py: update is
 * this operation on the host.
 *   elmk_accum_add     register an entry; returns its index (>= 0, in order of registration).  Allocates the value rows, zero-filled,
 *                      with n = 0 (counted in elmk_device_bytes, with the 16 KiB row table of the first entry).  dst_field = -1: no
 *                      destination.  A destination must be an F64 field of the source's nlev and of class SURFACE (nothing else may
 *                      own it), not the destination of another entry and not the entry's own source.  No entry reads what another
 *                      writes: a destination may not be the source of another entry, nor a source the destination of one (the rows
 *                      of all entries run in one launch, in no order).  ELMK_E_INVALID, nothing changed: a bad field, kind or
 *                      period, such a destination or source, a full table (ELMK_ACCUM_MAX_ENTRIES), a stream being captured.
 *   elmk_accum_init    set val from host[nlev][ncols] (SoA) and n = nsteps >= 0: how a restart file's T10 and nstep come in.  host =
 *                      NULL: val is seeded from the destination field's current contents (widened), ELMK_E_INVALID without a
 *                      destination.  Synchronises, as elmk_upload does.
 *   elmk_accum_update  fold the current state into every entry: stream-ordered and capturable, no host memory, no synchronisation;
 *                      writes nothing but value rows, counts and destination fields.  Two launches (the update of every row of every
 *                      entry, then a one-thread kernel that advances the counts); nothing without entries.  A captured graph holds
 *                      the entry table of the moment of capture: capture again after add / clear.
 *   elmk_accum_read    val of columns [col0, col0 + n) as doubles, layout as elmk_download (host may be NULL with n = 0), and the
 *                      count (nsteps may be NULL); synchronises.
 *   elmk_accum_clear   drop every entry and free its buffers; destination fields keep their values.
 * elmk_run with ELMK_RUN_ACCUM runs the update in every step, after elmk_advance_physics and the step's conservation and flag rows and
 * before elmk_history_accumulate (ELM's order: a tape of t10 sees the new value); graph on and off give the same bits.
 * A context without entries runs the kernels, launch sequences and graphs it ran before, allocates nothing more and saves the
 * restart image it saved before. */
enum { ELMK_ACCUM_RUNMEAN = 0, ELMK_ACCUM_TIMEAVG = 1, ELMK_ACCUM_RUNACCUM = 2 };
#define ELMK_ACCUM_MAX_ENTRIES 16
int elmk_accum_add(elmk_ctx *ctx, int src_field, int kind, int64_t period_steps, int dst_field);
int elmk_accum_init(elmk_ctx *ctx, int entry, const double *host /*[nlev][ncols] SoA, or NULL*/, int64_t nsteps);
int elmk_accum_update(elmk_ctx *ctx);
int elmk_accum_read(elmk_ctx *ctx, int entry, double *host, int64_t col0, int64_t n, int layout, int64_t *nsteps);
int elmk_accum_clear(elmk_ctx *ctx);

/* ---- aerosol deposition -----------------------------------------------------------------------
 * The eleven deposition streams aer_bcphi .. aer_dst4_2 (aero_data::AerosolFileInput, src/data/aerosol_data.h:10-28; kg/m2/s) are
 * what snow hydrology's compute_aerosol_deposition reads every step to grow the snow aerosol masses mss_*, which SNICAR turns into
 * snow albedo.  No kernel of the step writes them: without these calls they keep whatever was uploaded, and a long elmk_run has no
 * dust season.  ELM holds the input as twelve monthly records per stream on the aerosol file's own coarse grid (1.9 x 2.5 deg) and
 * interpolates every stream in time every step (aerdepini / aerinterp); the reference has the hook commented out at
 * init_timestep_kokkos.cc:48-49 (aerosol_data_old_impl.hh:32-55: the month bracket of monthly_data and a nearest-cell pick).  Here
 * the twelve months of every stream live on the device, on a grid of their own, and one kernel writes the eleven fields.
 * For every stream s (field ELMK_FIELD_aer_bcphi + s, AerosolFileInput's member order) and column c, without contraction:
 *   r1 = remap of cells x[s][month1] to column c;  r2 = remap of cells x[s][month2] to column c
 *   aer_s[c] = wt1 * r1 + wt2 * r2
 * - two products and one sum, as written also when month1 == month2 or a weight is 0 or 1: weights (1, 0) give x * 1 + y * 0, not a
 * copy, so a NaN or infinity in the other month propagates (NaN * 0 = NaN) and -0.0 * 1 + x * 0 is +0.0.  The remap is
 * elmk_set_forcing_grid's, in its operation order (regrid.apply_map): v = w[0][c] * a[idx[0][c]], then for k = 1 .. npts-1, if
 * idx[k][c] >= 0, v = v + w[k][c] * a[idx[k][c]]; idx = -1 is padding, skipped and never multiplied.  Without a map (per-column
 * series) r = x[s][month][c] itself.  The result is stored at state precision (rounded to fp32 in libelmk_f32.so, as elmk_upload
 * rounds).  Every stream is interpolated on its own, as aerinterp does; the sums bcpho + bcdep, dstX_1 + dstX_2 and the * dtime stay
 * in snow hydrology (aerosol_physics_impl.hh:49-57).  elmkernels_amd/aerosol.py: interpolate is this operation on the host.
 *   elmk_aerosol_reserve     allocates the cell series [11][12][ncells], fp64 in both builds (a few MB: one arithmetic for both),
 *                            zero-filled, and keeps a map of the aerosol grid in the ELL form, padding and validation of
 *                            elmk_set_forcing_grid: idx[npts][ncols] / w[npts][ncols] copied, npts 1 .. 8 stored as npad = 1, 2, 4
 *                            or 8 rows (regrid.nearest_map: the reference's nearest-cell pick; regrid.bilinear_map: what ELM's
 *                            stream mapping does).  idx == NULL and w == NULL: per-column series, ncells must equal ncols, npts is
 *                            ignored and no map is stored.  Independent of the forcing grid and of the run reservation: setting or
 *                            clearing it releases neither.  Waits for the runs in flight, drops the captured run step (the next
 *                            elmk_run under elmk_set_graph captures again) and replaces an earlier reservation, series included.
 *                            ELMK_E_INVALID, nothing enqueued: only one of idx, w NULL; ncells outside 1 .. 2^31-1; ncells != ncols
 *                            without a map; npts outside 1 .. 8; idx[0][c] outside [0, ncells); idx[k][c] outside [-1, ncells) for
 *                            k >= 1; a non-finite weight where idx >= 0; a stream being captured.
 *                            Device memory (elmk_device_bytes): 11 x 12 x ncells x 8 bytes for the series and, with a map, npad x 4
 *                            bytes x elmk_level_stride (idx) and npad x 8 bytes x elmk_level_stride (w), each of the three rounded
 *                            up to 256 bytes.
 *   elmk_aerosol_upload      months [month0, month0 + nmonths) of one stream from host[nmonths][ncells], record-major.  The copy runs
 *                            on the internal copy stream, so it overlaps a run in flight; it first waits for every enqueued,
 *                            unfinished reader of those months (an elmk_run with ELMK_RUN_AEROSOL whose steps name one of them, any
 *                            elmk_aerosol_deposition) and returns when the copy is done: elmk_series_upload's contract.
 *                            ELMK_E_INVALID: no reservation, a field that is not one of the eleven, month0 < 0, nmonths < 1,
 *                            month0 + nmonths > 12, host NULL, a stream being captured.
 *   elmk_aerosol_deposition  one kernel launch that writes all eleven fields of every column and touches nothing else; stream-ordered,
 *                            no synchronisation.  Picking the months and weights is date arithmetic and stays with the caller, as
 *                            for elmk_phenology (monthly_data.cc:29-62); the reference's commented call would pass the step-centred
 *                            date.  ELMK_E_INVALID, nothing enqueued: no reservation, a month outside 0 .. 11, a non-finite weight,
 *                            a stream being captured (it is captured only as part of elmk_run's own step).
 *   elmk_aerosol_clear       free the series and the map; aer_* keep their values.  Waits and drops the captured step as the reserve.
 * elmk_run with ELMK_RUN_AEROSOL runs the same kernel in every step between the forcing kernel and elmk_init_timestep, where the
 * reference's hook sits, with month1, month2, month_wt1, month_wt2 of the step's row.  This is a decision: elmk_run_step does not grow,
 * the aerosol interpolation uses the PHENOLOGY bracket of the step (the step-start date's), not a step-centred bracket of its own.  A
 * run with the flag overwrites aer_* and gives, bit for bit and with the graph on or off, the stepwise calls with
 * elmk_aerosol_deposition(month1, month2, month_wt1, month_wt2) before elmk_init_timestep; without the flag aer_* are read-only, as
 * they were.  ELMK_E_INVALID before anything is enqueued for the flag without a reservation.
 * Restart: aer_* are SURFACE fields, so an image carries them.  The series are an input like the forcing series and are not in the
 * image: reserve and upload again after elmk_restart_load.  The image format does not change.
 * A context that never calls these runs the kernels, launch sequences and graphs it ran before and allocates nothing more. */
int elmk_aerosol_reserve(elmk_ctx *ctx, int64_t ncells, int npts, const int32_t *idx /*[npts][ncols] or NULL*/,
                         const double *w /*[npts][ncols] or NULL*/);
int elmk_aerosol_upload(elmk_ctx *ctx, int field /*ELMK_FIELD_aer_bcphi .. ELMK_FIELD_aer_dst4_2*/, int month0, int nmonths,
                        const double *host /*[nmonths][ncells]*/);
int elmk_aerosol_deposition(elmk_ctx *ctx, int month1, int month2, double wt1, double wt2);
int elmk_aerosol_clear(elmk_ctx *ctx);

/* ---- active layer thickness --------------------------------------------------------------------
 * ELM's ActiveLayerMod::alt_calc on the device: the depth of the thaw front (history fields ALT, ALTMAX, ALTMAX_LASTYEAR) and the
 * two layer indices altmax_indx and altmax_lastyear_indx, which initialize_flux -> calc_root_moist_stress -> normalize_unfrozen_rootfr
 * reads every step.  The reference marks both fields NEED!! (src/data/elm_state_impl.hh:274-276) and has no alt_calc; no kernel of the
 * step writes them, so without these calls they keep what was uploaded (the reference driver's placeholders are 5 and 0).  ELM runs the
 * routine once per step after the soil temperature solve.  The feature owns three fp64 rows [level stride] (in both builds): alt,
 * altmax, altmax_lastyear (ELMK_ALT_*); the indices are the two I32 state fields.
 * One update, per column c, with t[j] and z[j] the temperature and node depth of soil layer j = 0 .. 14 (level 5 + j of t_soisno / zsoi,
 * widened to fp64), tfrz = 273.15, without contraction (`/` is the correctly rounded fp64 division):
 *   if (roll_c) { altmax_lastyear = altmax;  altmax_lastyear_indx = altmax_indx;  altmax = +0.0;  altmax_indx = -1; }
 *   if (t[14] > tfrz) { a = z[14];  k = 14; }
 *   else { k = the largest j in 0 .. 13 with t[j] > tfrz, or -1 if there is none      (from the bottom upward: a talik counts)
 *          if (k >= 0) a = z[k] + ((t[k] - tfrz) * (z[k+1] - z[k])) / (t[k] - t[k+1]);  else a = +0.0; }
 *   if (a != a) a = the canonical quiet NaN, bits 0x7FF8000000000000;
 *   alt = a;  if (a > altmax) { altmax = a;  altmax_indx = k; }
 * Every comparison is the plain IEEE `>`: a NaN temperature is "not thawed", a NaN a is stored in alt and leaves altmax alone; no error
 * bit is raised.  A NaN a (from a NaN or infinite t or z) is stored as that one NaN: IEEE 754 leaves the sign and payload of a NaN result
 * to the implementation, and device and host arithmetic differ there, so the operation fixes them.  The indices are 0-BASED soil-layer numbers with -1 for "no thawed layer", that is ELM's index minus one: the only
 * consumer reads them as i <= max(0, max(altmax_lastyear_indx, altmax_indx)) over 0-based i (soil_moist_stress_impl.hh:41), which is
 * ELM's j <= max(indx, 1) over 1-based j.  The annual rollover (ELM: before the search) is per hemisphere:
 *   roll_c = (rollover & ELMK_ALT_ROLL_NORTH) && north_c || (rollover & ELMK_ALT_ROLL_SOUTH) && !north_c,
 *   north_c = geo[ELMK_GEO_SIN_LAT][c] > 0.0 - for |lat| <= pi/2 ELM's lat > 0, with lat == 0 going south.
 * elmkernels_amd/active_layer.py: update is this operation on the host.
 *   elmk_active_layer_enable  allocates the three rows, zero-filled (one owner of 3 x 8 bytes x elmk_level_stride, counted in
 *                             elmk_device_bytes); writes no state field; drops the captured run step.  ELMK_E_INVALID, nothing
 *                             changed: already enabled; a stream being captured.
 *   elmk_active_layer_init    altmax and altmax_lastyear from host[ncols] each (NULL: zeros), alt = zeros: how a restart file's ALTMAX
 *                             comes in (the indices come in through elmk_upload).  Synchronises.
 *   elmk_active_layer_update  one launch; stream-ordered and capturable, no host memory, no synchronisation; writes nothing but the
 *                             three rows and the two index fields.  ELMK_E_INVALID, nothing enqueued: not enabled; no column
 *                             geography; unknown rollover bits.
 *   elmk_active_layer_read    row `which` (ELMK_ALT_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_active_layer_clear   frees the rows and drops the captured run step; the state fields keep their values.
 * elmk_run with ELMK_RUN_ALT runs the update in every step, after the step's conservation and flag rows and before the accumulated
 * fields and the history (ELM's order: tapes and accumulators of the index fields see the new values); refused before anything is
 * enqueued when not enabled.  The step's rollover is derived on the host from the step's start date, in the reference's no-leap
 * calendar: NORTH iff doy == 0 && decday == 1.0 (the step that starts at 00:00 of 1 January), SOUTH iff doy == 181 && decday == 182.0
 * (1 July) - the step whose end-of-step date satisfies ELM's mon, day == 1 && sec / dtime == 1 (active_layer.rollover).  Graph on and
 * off give the same bits.
 * Restart: a context with the feature enabled saves a version-3 image that carries the three rows ("restart" below).
 * A context that never enables the feature runs the kernels, launch sequences and graphs it ran before, allocates nothing more and
 * saves the image it saved before. */
enum { ELMK_ALT_ALT = 0, ELMK_ALT_ALTMAX = 1, ELMK_ALT_ALTMAX_LASTYEAR = 2 };
enum { ELMK_ALT_ROLL_NORTH = 1, ELMK_ALT_ROLL_SOUTH = 2 };
#define ELMK_RUN_ALT 16 /* the fifth flag bit of elmk_run: every step updates the active layer thickness */
int elmk_active_layer_enable(elmk_ctx *ctx);
int elmk_active_layer_init(elmk_ctx *ctx, const double *altmax /*[ncols] or NULL*/, const double *altmax_lastyear /*[ncols] or NULL*/);
int elmk_active_layer_update(elmk_ctx *ctx, int rollover /*ELMK_ALT_ROLL_* bits*/);
int elmk_active_layer_read(elmk_ctx *ctx, int which, double *host, int64_t col0, int64_t n);
int elmk_active_layer_clear(elmk_ctx *ctx);

/* ---- soil hydrology -------------------------------------------------------------------------------
 * ELM v1's column soil hydrology in the CLM4.5 formulation, as one opt-in stage at the end of the step: surface runoff, infiltration
 * with the h2osfc store, the Zeng-Decker Richards solve with the aquifer as an extra row, the water-table update and drainage.  The
 * reference has none of it: its conservation row hardwires hydrology_source_sink = 0.0 (driver/kokkos/conserved_quantity_kokkos.cc:22)
 * and it expects an external subsurface model, so without this stage no kernel applies qflx_top_soil, qflx_rootsoi or the ground
 * evaporation terms to the soil layers.  Out of scope: VSFM, lakes, wetlands, urban (lateral flow and irrigation: the sections of those names below).
 * This text is the specification; elmkernels_amd/hydrology.py: column() is the same operation on the host, and where an evaluation
 * order is not spelled out here that function fixes it (k_soil_hydrology.hip follows it statement by statement, bit for bit).
 *
 * Conventions.  pow, exp: glibc's (elmk_pow, elmk_exp on the device); 10^x is pow(10.0, x).  No contraction; `/` is the correctly
 * rounded fp64 division; comparisons are plain IEEE; min(a, b) = (b < a ? b : a), max(a, b) = (a < b ? b : a); a * b * c and a / b / c
 * associate from the left.  N = ELMK_HYD_NLAYER = 10 layers are active: layer j is level 5 + j of h2osoi_liq, h2osoi_ice, dz, zsoi and
 * level j of watsat, sucsat, bsw, h2osoi_vol, qflx_rootsoi; zi[j] is level 6 + j of zisoi and zi[-1] level 5 (the surface); layers
 * 10 .. 14 are never touched.  denh2o = 1000, denice = 917, e_ice = 6, smpmin = -1e8, watmin = 0.01, pc = 0.4, mu = 0.13889,
 * fff_s = 0.5, fff_d = 2.5, aquifer_max = 5000, rous_min = 0.02; zmm, zimm, dzmm, zwtmm = zsoi, zi, dz, zwt times 1e3.  State fields
 * are widened to fp64 as stored, and a result is rounded once to the stored type.
 *
 * The feature owns ELMK_HYD_NROWS fp64 rows [level stride] (in both builds): prognostic ZWT (m), WA (mm); parameters HKSAT[10] (mm/s),
 * WTFACT, H2OSFC_THRESH (mm), K_WET, RSUB_TOP_MAX (mm/s); diagnostics, overwritten every step, QFLX_SURF, QFLX_INFL,
 * QFLX_H2OSFC_SURF, QFLX_DRAIN, QFLX_RSUB_SAT, QCHARGE, FSAT.
 *
 * Per column, with dt and fsno = frac_sno_eff:
 * A. for j < N: vol_ice = min(watsat, ice / (dz * denice)); effpor = max(0.01, watsat - vol_ice); icefrac = min(1, vol_ice / watsat);
 *    vol_liq = max(liq, 1e-6) / (dz * denh2o); vol = liq / (dz * denh2o) + ice / (dz * denice).
 * B. fsat = wtfact * exp(-0.5 * fff_s * zwt); qflx_surf = fsat * qflx_top_soil.
 * C. qevap = snl == 0 ? qflx_evap_grnd : qflx_ev_soil;
 *    q_in_soil = (1 - frac_h2osfc) * (qflx_top_soil - qflx_surf); q_in_soil = q_in_soil - (1 - fsno - frac_h2osfc) * qevap;
 *    q_in_sfc = frac_h2osfc * (qflx_top_soil - qflx_surf); q_in_sfc = q_in_sfc - frac_h2osfc * qflx_ev_h2osfc;
 *    m = pow(10, -e_ice * icefrac[0]) * hksat[0]; m = min(m, the same of layer 1); m = min(m, of layer 2); qinmax = (1 - fsat) * m;
 *    excess = max(0, q_in_soil - (1 - frac_h2osfc) * qinmax); infl = q_in_soil - excess; q_in_sfc = q_in_sfc + excess;
 *    frac_infclust = frac_h2osfc <= pc ? 0 : pow(frac_h2osfc - pc, mu);
 *    qs = h2osfc >= thresh ? min(k_wet * frac_infclust * (h2osfc - thresh), (h2osfc - thresh) / dt) : 0; if (qs < 1e-8) qs = 0;
 *    h2osfc = h2osfc + (q_in_sfc - qs) * dt;
 *    if (h2osfc < 0) { infl = infl + h2osfc / dt; h2osfc = 0; drain_sfc = 0; } else drain_sfc = min(frac_h2osfc * qinmax, h2osfc / dt);
 *    h2osfc = h2osfc - drain_sfc * dt; infl = infl + drain_sfc.        (qs is the diagnostic QFLX_H2OSFC_SURF)
 * D. 1. jwt = the first j with zwt <= zi[j], else N.
 *    2. for j < N, b1 = 1 - 1 / bsw:  zwtmm <= zimm[j-1]: ve = watsat;
 *       else zwtmm < zimm[j]: t0 = pow((sucsat + zwtmm - zimm[j-1]) / sucsat, b1);
 *            v1 = -sucsat * watsat / b1 / (zwtmm - zimm[j-1]) * (1 - t0);
 *            ve = (v1 * (zwtmm - zimm[j-1]) + watsat * (zimm[j] - zwtmm)) / (zimm[j] - zimm[j-1]);
 *       else ti = pow((sucsat + zwtmm - zimm[j]) / sucsat, b1); t0 as above; ve = -sucsat * watsat / b1 / (zimm[j] - zimm[j-1]) * (ti - t0);
 *       ve = min(watsat, max(ve, 0)); zq[j] = max(smpmin, -sucsat * pow(max(ve / watsat, 0.01), -bsw)).
 *    3. only if jwt == N, with layer N-1's parameters: t0 and v1 as in the middle case over [zimm[N-1], zwtmm]; ve = v1 (the layer ends at
 *       the water table, as in ELM), clamped as above; zq[N] from it; zmm[N] = 0.5 * (zwtmm + zmm[N-1]); dzmm[N] = zwtmm - zimm[N-1].
 *    4. jp = min(N-1, j+1): s1 = min(1, 0.5 * (vol[j] + vol[jp]) / (0.5 * (watsat[j] + watsat[jp]))); s2 = hksat[j] * pow(s1, 2 * bsw[j] + 2);
 *       imped[j] = pow(10, -e_ice * (0.5 * (icefrac[j] + icefrac[jp]))); hk[j] = imped * s1 * s2;
 *       dhkdw[j] = imped * (2 * bsw[j] + 3) * s2 * (1 / (watsat[j] + watsat[jp])).
 *    5. sn = min(1, max(vol_liq[j] / watsat[j], 0.01)); smp[j] = max(smpmin, -sucsat * pow(sn, -bsw)); dsmpdw[j] = -bsw * smp / (sn * watsat);
 *       aquifer (jwt == N): sn1 = min(1, max(vol[N-1] / watsat[N-1], 0.01)), smp1 and dsmpdw1 from it with layer N-1's parameters.
 *    6. interface i between nodes i and i+1, i = 0 .. N-2: den = zmm[i+1] - zmm[i]; num = (smp[i+1] - smp[i]) - (zq[i+1] - zq[i]);
 *       q[i] = -hk[i] * num / den; dq1[i] = -(-hk[i] * dsmpdw[i] + num * dhkdw[i]) / den; dq2[i] = -(hk[i] * dsmpdw[i+1] + num * dhkdw[i]) / den.
 *       Interface N-1: with jwt == N the same against the aquifer node (zmm[N], zq[N], smp1, dsmpdw1; hk[N-1], dhkdw[N-1]); else all 0.
 *    7. rows: r[0] = infl - q[0] - rootsoi[0], a[0] = 0, b[0] = dzmm[0] / dt + dq1[0], c[0] = dq2[0];
 *       j = 1 .. N-1: r = q[j-1] - q[j] - rootsoi[j], a = -dq1[j-1], b = dzmm[j] / dt - dq2[j-1] + dq1[j], c = dq2[j];
 *       row N: jwt == N: r = q[N-1], a = -dq1[N-1], b = dzmm[N] / dt - dq2[N-1], c = 0; else r = 0, a = 0, b = 1, c = 0.
 *    8. Thomas: bet = b[0]; u[0] = r[0] / bet; for j = 1 .. N: gam[j] = c[j-1] / bet; bet = b[j] - a[j] * gam[j];
 *       u[j] = (r[j] - a[j] * u[j-1]) / bet;   then for j = N-1 .. 0: u[j] = u[j] - gam[j+1] * u[j+1].
 *    9. liq[j] = liq[j] + u[j] * dzmm[j], j < N.
 *    10. jwt == N: qcharge = u[N] * dzmm[N] / dt.  Else k = jwt, up = max(0, jwt - 1), from the values before the solve:
 *        sn = max(vol[k] / watsat[k], 0.01); ka = imped[k] * hksat[k] * pow(min(1, sn), 2 * bsw[k] + 3); wh = smp[up] - zq[up];
 *        qcharge = jwt == 0 ? -ka * (0 - wh) / ((zwt + 1e-3) * 1000) : -ka * (0 - wh) / ((zwt - zsoi[jwt-1]) * 1000 * 2);
 *        qcharge = max(-10 / dt, qcharge); qcharge = min(10 / dt, qcharge).
 * E. sy(j) = max(rous_min, watsat[j] * (1 - pow(1 + 1e3 * zwt / sucsat[j], -1 / bsw[j]))) with the zwt current where it is evaluated;
 *    rous = sy(N-1) at the start of E.  jwt == N: wa = wa + qcharge * dt; zwt = zwt - qcharge * dt / 1000 / rous.  Else qt = qcharge * dt;
 *    qt > 0: for j = jwt down to 0: ql = max(0, min(qt, sy(j) * (zwt - zi[j-1]) * 1e3)); zwt = zwt - ql / sy(j) / 1000 (the same sy);
 *            qt = qt - ql; stop when qt <= 0.
 *    else:   for j = jwt .. N-1: ql = min(0, max(qt, -(sy(j) * (zi[j] - zwt) * 1e3))); qt = qt - ql;
 *            if (qt >= 0) { zwt = zwt - ql / sy(j) / 1000; stop; } else zwt = zi[j];     after the walk: if (qt < 0) zwt = zwt - qt / 1000 / rous.
 *    Then jwt is recomputed.
 * F. 1. rous = sy(N-1) again (ELM's Drainage recomputes it); imp = pow(10, -e_ice * (si / sd)), si = sum of icefrac * dzmm and sd = sum
 *       of dzmm over j = max(jwt-1, 0) .. N-1, each from 0.0 in ascending j; rsub_top = imp * rsub_top_max * exp(-fff_d * zwt);
 *       rt = -rsub_top * dt.
 *    2. jwt == N: wa = wa + rt; zwt = zwt - rt / 1000 / rous; liq[N-1] = liq[N-1] + max(0, wa - aquifer_max); wa = min(wa, aquifer_max).
 *       Else the falling walk of E with rt for qt and liq[j] = liq[j] + ql in every visited layer, then (always) zwt = zwt - rt / 1000 / rous
 *       and wa = wa + rt with the rt that is left.
 *    3. zwt = zwt < 0 ? 0 : zwt; zwt = 80 < zwt ? 80 : zwt   (a NaN stays).
 *    4. j = N-1 down to 1: cap = effpor[j] * dzmm[j]; xs = max(liq[j] - cap, 0); liq[j] = min(cap, liq[j]); liq[j-1] = liq[j-1] + xs.
 *    5. xs1 = max(max(liq[0], 0) - max(0, watsat[0] * dzmm[0] - ice[0]), 0); liq[0] = liq[0] - xs1; h2osfc = h2osfc + xs1; rsub_sat = 0.
 *    6. j = 0 .. N-2: if (liq[j] < watmin) { xs = watmin - liq[j]; liq[j] = liq[j] + xs; liq[j+1] = liq[j+1] - xs; }
 *    7. if (liq[N-1] < watmin) { xs = watmin - liq[N-1]; for i = N-2 down to 0 while xs > 0: avail = max(liq[i] - watmin - xs, 0);
 *       take = min(avail, xs); liq[N-1] = liq[N-1] + take; liq[i] = liq[i] - take; xs = max(xs - take, 0);   then
 *       liq[N-1] = liq[N-1] + xs; rsub_top = rsub_top - xs / dt; }
 *    8. qflx_drain = rsub_sat + rsub_top.
 * F'. The frost table and the perched water table, in place of F.1 and F.2 from elmk_soil_hydrology_frost_enable on (F.3 to F.8, G and H
 *    are unchanged).  In this part layers are 0-based, zi[j] is the bottom of layer j and z[j] is zsoi of layer j.  t[j] is level 5 + j of
 *    t_soisno, widened to fp64 as stored; tfrz = 273.15, sat_lev = 0.9; q_perch_max is a per-column parameter row (1/s); imped[j] is
 *    D.4's value, from the ice before the solve; effpor and icefrac are A's values; liq is the current value, after D.9; ice is as read.
 *    0. rous = sy(N-1), as in F.1.  kf = t[0] > tfrz ? N-1 : 0; for k = 1 .. N-1 ascending: at the first k with t[k-1] > tfrz &&
 *       t[k] <= tfrz, kf = k and stop.  ft = z[kf]; frozen = t[kf] <= tfrz; zwp = ft; qp = 0.
 *    A. taken if zwt < ft && frozen (the water table is above the frost table; jwt <= kf follows):
 *       qs = 0.0; ws = 0.0; for j = jwt .. kf ascending: qs = qs + imped[j] * hksat[j] * dzmm[j]; ws = ws + dzmm[j];
 *       if (ws > 0) qs = qs / ws; qp = q_perch_max * qs * (ft - zwt); rt = -qp * dt;
 *       for j = jwt .. kf ascending: rl = max(rt, -(liq[j] - watmin)); rl = min(rl, 0); rt = rt - rl; liq[j] = liq[j] + rl;
 *           if (rt >= 0) { zwt = zwt - rl / effpor[j] / 1000; stop; } else zwt = zi[j];
 *       after the walk: qp = qp + rt / dt.  rsub_top = 0; F.1's rsub_top and all of F.2 are skipped; wa is unchanged; jwt is recomputed.
 *    B. taken otherwise (a NaN zwt lands here).  v(k) = liq[k] / (dz[k] * denh2o) + ice[k] / (dz[k] * denice).
 *       kp = 0; for k = kf down to 0: at the first k with v(k) / watsat[k] <= sat_lev, kp = k and stop.  if (!frozen) kp = kf.
 *       If kf > kp: s1 = v(kp) / watsat[kp]; s2 = v(kp+1) / watsat[kp+1]; m = (z[kp+1] - z[kp]) / (s2 - s1); b = z[kp+1] - m * s2;
 *           zwp = max(0, m * sat_lev + b) (with the max above a NaN gives 0); qs, ws as in A over j = kp .. kf, with the same if (ws > 0);
 *           qp = q_perch_max * qs * (ft - zwp); rt = -qp * dt; the walk of A over j = kp+1 .. kf with zwp in the place of zwt;
 *           qp = qp + rt / dt.
 *       Then F.1 (imp, rsub_top, rt) and F.2, exactly as above, on the liq the removal left.
 *    Stores, in addition to H's: FROST_TABLE = ft, ZWT_PERCHED = zwp, QFLX_DRAIN_PERCHED = qp; a NaN is stored as the canonical quiet NaN.
 *    Two consequences: a column whose ten t are all above tfrz, or whose only frozen layer is layer 0 with zwt >= z[0], takes B with
 *    kp == kf, and its A to H outputs are the bits of the stage without the extension; with q_perch_max == 0 every column of B has the
 *    bits of the stage without the extension in every A to H output (the removals add -0.0).
 * G. where snl == 0: liq[0] = liq[0] + (1 - frac_h2osfc) * qflx_dew_grnd * dt; ice[0] = ice[0] + (1 - frac_h2osfc) * qflx_dew_snow * dt;
 *    if (qflx_sub_snow * dt > ice[0]) ice[0] = 0; else ice[0] = ice[0] - (1 - frac_h2osfc) * qflx_sub_snow * dt.
 * H. h2osoi_vol[j] = liq / (dz * denh2o) + ice / (dz * denice) from the new fp64 values, j < N.  The stage writes h2osoi_liq (layers
 *    0 .. N-1), h2osoi_ice (layer 0, where snl == 0), h2osoi_vol, h2osfc, ZWT, WA and the seven diagnostic rows.  A NaN stored into a row of
 *    the feature is the canonical quiet NaN (bits 0x7FF8000000000000), as in the active layer thickness.  No error bit is raised.
 *
 *   elmk_soil_hydrology_enable      allocates the rows, zero-filled (ELMK_HYD_NROWS x 8 bytes x elmk_level_stride, counted in
 *                                   elmk_device_bytes); drops the captured run step.  ELMK_E_INVALID, nothing changed: already enabled;
 *                                   a stream being captured.
 *   elmk_soil_hydrology_set_params  the parameter rows from the host: hksat[10][ncols] (layer-major) and four [ncols] rows.  Synchronises.
 *   elmk_soil_hydrology_init        ZWT and WA from host[ncols] each; NULL for either means ELM's cold start, wa = 4000 and
 *                                   zwt = (zi[9] + 25) - 4000 / 0.2 / 1000 from the column's zisoi (hydrology.cold_start_zwt).  Synchronises.
 *   elmk_soil_hydrology             one launch; stream-ordered and capturable, no host memory, no synchronisation.  ELMK_E_INVALID,
 *                                   nothing enqueued: not enabled; parameters never set; dt not finite and positive.  A context whose
 *                                   land unit (elmk_set_land) is not soil or crop enqueues nothing and returns ELMK_OK.
 *   elmk_soil_hydrology_read        row `which` (ELMK_HYD_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_soil_hydrology_clear       frees the rows and drops the captured run step; the state fields keep their values.
 * The frost-table extension owns ELMK_HYDF_NROWS fp64 rows of its own [level stride]: the parameter Q_PERCH_MAX (1/s;
 * hydrology.q_perch_max: 1e-5 sin(slope), evaluated on the host) and the diagnostics FROST_TABLE (m), ZWT_PERCHED (m) and
 * QFLX_DRAIN_PERCHED (mm/s), overwritten every step.  ELMK_HYD_NROWS and the rows above stay what they are.
 *   elmk_soil_hydrology_frost_enable  allocates the rows (ELMK_HYDF_NROWS x 8 bytes x elmk_level_stride, counted in elmk_device_bytes),
 *                                     uploads q_perch_max[ncols], zero-fills the diagnostics and drops the captured run step.  From here
 *                                     on elmk_soil_hydrology, and elmk_run with ELMK_RUN_HYDROLOGY, take the F' form: there is no flag
 *                                     of its own.  ELMK_E_INVALID, nothing changed: the hydrology is not enabled; already enabled; a
 *                                     null argument; a stream being captured.
 *   elmk_soil_hydrology_frost_read    row `which` (ELMK_HYDF_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_soil_hydrology_frost_clear   frees these rows only and drops the captured run step: the stage is F again.
 *                                     elmk_soil_hydrology_clear frees them too.
 * The three diagnostics are recomputed from scratch every step and the parameter stays with the driver, so the restart image of a
 * context with the extension is byte for byte the size of the version-4 image, and N + N steps across a restart equal 2N.
 * elmk_run with ELMK_RUN_HYDROLOGY runs the stage in every step after elmk_surface_fluxes and before the step's conservation row (whose
 * errh2o keeps the reference's hardwired source_sink = 0; the closed budget is the stage of "water balance" below); refused before anything is
 * enqueued when not enabled or without parameters.  Graph on and off give the same bits.
 * Restart: a context with the feature enabled saves a version-4 image that carries ZWT and WA ("restart" below); the parameter rows
 * stay with the driver, like the geography.  A context that never enables the feature runs the kernels, launch sequences and graphs
 * it ran before, allocates nothing more and saves the image it saved before. */
#define ELMK_HYD_NLAYER 10
enum {
  ELMK_HYD_ZWT = 0, ELMK_HYD_WA = 1, ELMK_HYD_HKSAT = 2 /* .. 11 */, ELMK_HYD_WTFACT = 12, ELMK_HYD_H2OSFC_THRESH = 13, ELMK_HYD_K_WET = 14,
  ELMK_HYD_RSUB_TOP_MAX = 15, ELMK_HYD_QFLX_SURF = 16, ELMK_HYD_QFLX_INFL = 17, ELMK_HYD_QFLX_H2OSFC_SURF = 18, ELMK_HYD_QFLX_DRAIN = 19,
  ELMK_HYD_QFLX_RSUB_SAT = 20, ELMK_HYD_QCHARGE = 21, ELMK_HYD_FSAT = 22, ELMK_HYD_NROWS = 23
};
#define ELMK_RUN_HYDROLOGY 32 /* the sixth flag bit of elmk_run: every step runs the soil hydrology stage */
int elmk_soil_hydrology_enable(elmk_ctx *ctx);
int elmk_soil_hydrology_set_params(elmk_ctx *ctx, const double *hksat /*[10][ncols]*/, const double *wtfact /*[ncols]*/,
                                   const double *h2osfc_thresh /*[ncols]*/, const double *k_wet /*[ncols]*/,
                                   const double *rsub_top_max /*[ncols]*/);
int elmk_soil_hydrology_init(elmk_ctx *ctx, const double *zwt /*[ncols] or NULL*/, const double *wa /*[ncols] or NULL*/);
int elmk_soil_hydrology(elmk_ctx *ctx, double dt);
int elmk_soil_hydrology_read(elmk_ctx *ctx, int which, double *host, int64_t col0, int64_t n);
int elmk_soil_hydrology_clear(elmk_ctx *ctx);
enum { ELMK_HYDF_Q_PERCH_MAX = 0, ELMK_HYDF_FROST_TABLE = 1, ELMK_HYDF_ZWT_PERCHED = 2, ELMK_HYDF_QFLX_DRAIN_PERCHED = 3, ELMK_HYDF_NROWS = 4 };
int elmk_soil_hydrology_frost_enable(elmk_ctx *ctx, const double *q_perch_max /*[ncols]*/);
int elmk_soil_hydrology_frost_read(elmk_ctx *ctx, int which, double *host, int64_t col0, int64_t n);
int elmk_soil_hydrology_frost_clear(elmk_ctx *ctx);

/* ---- hillslope lateral flow ------------------------------------------------------------------------
 * The hillslope hydrology of CLM5 / CTSM (Swenson et al. 2019; SubsurfaceLateralFlow with use_hillslope): columns ordered along a
 * hillslope, Darcy flow between neighbours driven by the head difference, the lowest column discharging to the stream.  An opt-in
 * extension of the soil hydrology stage with no run flag and no restart-image change: while it is on, elmk_soil_hydrology and the
 * ELMK_RUN_HYDROLOGY stage enqueue two small launches (L1, L2) in front of the hydrology kernel and run its LAT form (L3).  The net
 * lateral flux takes the place of F.1's rsub_top, so QFLX_DRAIN, QRUNOFF and ERRH2O carry it as they are; the water balance and the
 * routing are unchanged.  The conventions are those of "soil hydrology": no contraction, elmk_pow, left association, that section's min
 * and max; zi[j] is the bottom of layer j.  elmkernels_amd/hydrology.py: hillslope_head, hillslope_flow and column() fix any evaluation
 * order this text leaves open.
 * The geometry, all [ncols]: down[c] >= 0 the downhill column; -1: the column's lower edge is the stream; -2: the column is on no
 * hillslope and keeps F.1's baseflow and the bits of the stage without the extension in every output.  dist: metres from the column's
 * centre to its downhill neighbour's centre, or to the stream; width: metres of the lower edge; area: square metres; elev: metres of
 * the surface above the stream's water surface.  k_aniso: the ratio of horizontal to vertical conductivity.
 * Host checks (elmk_maps.h: hillslope_check), in this order; on refusal nothing is changed and the message names the row and the first
 * offending column: the arguments; down in {-2, -1} or [0, ncols); no self-loop; no column draining into a -2 column; at most 8 columns
 * drain into one; no cycle (the linear two-mark walk of the river network's check, nothing recursive); dist, width, area finite and > 0
 * on hillslope columns; elev finite on hillslope columns; k_aniso finite and > 0.  The host builds the uphill map the device reads:
 * 1, 2, 4 or 8 rows, ascending uphill index per slot, -1 padding.
 *   L1 (launch 1, per column, from the values at the start of the stage: ZWT as stored, h2osoi_ice, dz, watsat, HKSAT, zi)
 *      down == -2: HEAD = 0; TRANS = 0.  Else icefrac as in A and jwt as in D.1;
 *      jwt == N: T = 0.  Else si, sd and imp = pow(10, -e_ice * (si / sd)) over j = max(jwt-1, 0) .. N-1 as in F.1;
 *        T = 0.0; for j = jwt .. N-1 ascending: T = T + hksat[j] * (j == jwt ? zi[j] - zwt : dz[j]);  T = imp * T * 1e-3 * k_aniso.
 *      HEAD = elev - zwt (m); TRANS = T (m2/s).
 *   L2 (launch 2, per column c).  The flux of the edge from u to d = down[u], m3/s:
 *        d == -1: g = max(HEAD[u] / dist[u], 0)  - the stream gives the land no water: there is no stream store yet;
 *        else     g = (HEAD[u] - HEAD[d]) / dist[u];
 *        g = min(max(g, -2), 2);  Td = (d != -1 && g < 0) ? TRANS[d] : TRANS[u];  vol(u) = Td * width[u] * g.
 *      QLAT_OUT[c] = 1e3 * vol(c) / area[c];  QLAT_IN[c] = the sum from 0.0, in slot order, of 1e3 * vol(u) / area[c] over the uphill
 *      slots, each vol(u) recomputed by c from the operands its owner uses, so both ends hold the same bits;  QLAT_NET = OUT - IN;
 *      QSTREAM = vol(c) where down == -1, else 0.  down == -2: all four 0.  A NaN is stored as the canonical quiet NaN.
 *   L3 (the hydrology kernel, columns with down != -2, in the place of F.1's rsub_top; rous as in F.1)
 *      rsub_top = QLAT_NET[c]; rt = -rsub_top * dt.  jwt == N: F.2 as it is.  Else, if rt > 0: E's rising walk with rt for qt and
 *      liq[j] = liq[j] + ql in every visited layer; afterwards liq[0] = liq[0] + rt with what is left; wa is untouched and rous is not
 *      applied.  Otherwise (a NaN included): F.2's falling walk as it is.  F.3 - F.8, G and H are unchanged; QFLX_DRAIN is then the net
 *      flux and may be negative.
 * Three consequences: a context whose columns are all -2 has the bits of a context without the extension in every field and row; a flat
 * hillslope (equal HEAD, the stream column's HEAD <= 0) has QLAT_* = 0 everywhere; over any hillslope sum(area * QLAT_NET) * 1e-3 equals
 * sum(QSTREAM) up to the roundings of L2's divisions and products.
 * The extension owns ELMK_HS_NROWS fp64 column rows [level stride], all recomputed every step: HEAD (m), TRANS (m2/s), QLAT_OUT, QLAT_IN,
 * QLAT_NET (mm/s), QSTREAM (m3/s, non-zero only where down == -1); beside them the geometry, down and the uphill map, all counted in
 * elmk_device_bytes.  Nothing of it is prognostic: the restart image of a context with the extension is byte for byte that of one
 * without, and N + N steps across a restart equal 2N once the driver has enabled the extension again.
 *   elmk_hillslope_enable   checks, allocates, uploads; drops the captured run step.  ELMK_E_INVALID, nothing changed: the hydrology
 *                           is not enabled; already on; a null argument; a refusal of the checks; a stream being captured; the frost
 *                           table is on (elmk_soil_hydrology_frost_clear first: F'.A skips F.1 and F.2, which would drop a flux the
 *                           neighbours have booked); the floodplain infiltration is on (elmk_floodplain_infiltration_clear first).
 *                           While the extension is on elmk_soil_hydrology_frost_enable and elmk_floodplain_infiltration_enable are
 *                           refused ("elmk_hillslope_clear first").
 *   elmk_hillslope_read     row `which` (ELMK_HS_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_hillslope_budget   sums[0] = the sum of QSTREAM through the conservation's reduction kernels; synchronises.
 *   elmk_hillslope_clear    frees everything of the extension and drops the captured run step: the stage is F again.  Refused while a
 *                           history or point-series entry reads its rows ("elmk_history_clear first").  elmk_soil_hydrology_clear
 *                           frees the extension too.
 * Tapes: ELMK_ROWS_HILLSLOPE (which = ELMK_HS_*) for elmk_column_history_add_row, elmk_gridded_history_add_row and the point series.
 * A context that never enables it runs the kernels, launch sequences and graphs it ran before, allocates nothing more and saves the image
 * it saved before.  Out of scope, later changes: a stream store coupled to the routing's channel depth (losing streams); the frost-table
 * and floodplain-infiltration combinations; per-layer ice impedance in the transmissivity; hillslope-dependent forcing. */
enum { ELMK_HS_HEAD = 0, ELMK_HS_TRANS = 1, ELMK_HS_QLAT_OUT = 2, ELMK_HS_QLAT_IN = 3, ELMK_HS_QLAT_NET = 4, ELMK_HS_QSTREAM = 5, ELMK_HS_NROWS = 6 };
int elmk_hillslope_enable(elmk_ctx *ctx, const int32_t *down /*[ncols]*/, const double *dist /*[ncols]*/, const double *width /*[ncols]*/,
                          const double *area /*[ncols]*/, const double *elev /*[ncols]*/, double k_aniso);
int elmk_hillslope_read(elmk_ctx *ctx, int which /*ELMK_HS_**/, double *host, int64_t col0, int64_t n);
int elmk_hillslope_budget(elmk_ctx *ctx, double *sums /*[1]: the sum of QSTREAM*/);
int elmk_hillslope_clear(elmk_ctx *ctx);

/* ---- water balance ---------------------------------------------------------------------------------
 * The closed column water budget of a step that runs the soil hydrology, and ELM's standard hydrology outputs.  The conservation row of
 * elmk_evaluate_conservation keeps the reference's hardwired hydrology_source_sink = 0.0 and knows nothing of the aquifer, so with the
 * hydrology every column that drains or runs off reports runoff * dt + (wa_end - wa_beg) there; that row stays bit for bit what it is.
 * This opt-in stage is the budget with the hydrology's fluxes and the aquifer in it.
 * This text is the specification; elmkernels_amd/hydrology.py: water_balance_begin / water_balance_end are the same operation on the
 * host, and k_water_balance.hip follows them statement by statement.
 *
 * Conventions, those of "soil hydrology": no contraction; +, -, * associate from the left; `/` is the correctly rounded fp64 division;
 * comparisons are plain IEEE; state fields are widened to fp64 as stored; the rows are fp64 in both builds; a NaN stored into a row is
 * the canonical quiet NaN.  Soil layer j is level 5 + j of h2osoi_liq, h2osoi_ice and dz; zi[j] is level 6 + j of zisoi and zi[-1]
 * level 5; N = ELMK_HYD_NLAYER.  WA, QFLX_* are the hydrology's rows, QFLX_DRAIN_PERCHED the frost-table extension's.
 *
 * The feature owns ELMK_WB_NROWS fp64 rows [level stride]: BEGWB, ERRH2O, QRUNOFF, ENDWB (ELM's TWS, with the aquifer in it),
 * SOILWATER_10CM, TOTSOILLIQ, TOTSOILICE (all mm, QRUNOFF mm/s).  ERRH2O, QRUNOFF, ENDWB are adjacent and in this order.
 *
 * Per column:
 * W0 (begin).  BEGWB = dtbegin_column_h2o + WA.
 * W1. water = h2ocan + h2osno + h2osfc; for i = 0 .. 19 ascending: water = water + (h2osoi_ice[i] + h2osoi_liq[i])   (the expression and
 *     order of the conservation row's column water mass).
 * W2. ENDWB = water + WA.
 * W3. q = QFLX_SURF + QFLX_H2OSFC_SURF + QFLX_DRAIN; with the frost-table extension enabled q = q + QFLX_DRAIN_PERCHED;
 *     QRUNOFF = q + qflx_snwcp_liq   (the liquid that snow capping removes, which ELM counts as qflx_qrgwl on soil columns; the
 *     reference's budget and hydrology.water_balance_error leave it out).
 * W4. ERRH2O = ENDWB - BEGWB - (forc_rain + forc_snow - QRUNOFF - qflx_evap_tot - qflx_snwcp_ice) * dt; while the irrigation is enabled
 *     (forc_rain + forc_snow) + QFLX_IRRIG takes the place of forc_rain + forc_snow ("irrigation" below).
 * W5. TOTSOILLIQ = the sum of liq[j], j = 0 .. N-1 ascending, from 0.0; TOTSOILICE the same over ice[j].  The library's own
 *     definition: the ten active layers; the bedrock levels are never touched by the stage.
 * W6. s = 0.0; for j = 0 .. N-1: if (zi[j] <= 0.1) s = s + (liq[j] + ice[j]);
 *     else if (zi[j-1] < 0.1) s = s + (liq[j] + ice[j]) * ((0.1 - zi[j-1]) / dz[j]);     SOILWATER_10CM = s.
 * W7. (min, max, sum) of ERRH2O, QRUNOFF and ENDWB over the context's columns, exactly in elmk_evaluate_conservation's contract: the same
 *     order of the sum, the same NaN-sticky min and max (diagnostics.reduce_min_max_sum).
 * W8. A column is bad iff !(fabs(ERRH2O) <= tol), so a NaN counts.  nbad is their count, first_bad_col the smallest bad index or -1.
 *     No error bit is raised.
 *
 *   elmk_water_balance_enable  allocates the rows, zero-filled, and the reduction's scratch (ELMK_WB_NROWS x 8 bytes x
 *                              elmk_level_stride and 36864 + 256 bytes, counted in elmk_device_bytes), and with a run reserved the
 *                              run's ring rows; drops the captured run step.  ELMK_E_INVALID, nothing changed: the soil hydrology is
 *                              not enabled; already enabled; tol_mm not finite or negative; a stream being captured.
 *   elmk_water_balance_begin   W0, one launch; stream-ordered and capturable.  After elmk_init_timestep, before the physics.
 *   elmk_water_balance         W1 - W8 after the step's elmk_soil_hydrology.  With all three pointers NULL stream-ordered and capturable
 *                              (the rows are written, the triples and the census stay on the device); otherwise it synchronises, as
 *                              elmk_evaluate_conservation does, and fills those given: min_max_sum[3][3] in the order ERRH2O, QRUNOFF,
 *                              ENDWB.  ELMK_E_INVALID, nothing enqueued: not enabled; dt not finite and positive.
 *   elmk_water_balance_read    row `which` (ELMK_WB_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_water_balance_clear   frees the rows, the scratch and the ring rows and drops the captured run step.  elmk_soil_hydrology_clear
 *                              frees them too.
 * A context whose land unit is not soil or crop enqueues nothing and reports what zero columns reduce to: +inf, -inf, +0.0; 0; -1.
 * elmk_run with ELMK_RUN_WATER_BALANCE: W0 runs right after the step's init_timestep, W1 - W8 after the step's flag-summary row and
 * before the active layer update, so accumulators and tapes see the new rows.  The triples, count and first column go into ring rows
 * of their own, double-buffered like the conservation ring and allocated only for a context that has the feature (at enable if a run
 * is reserved, at elmk_run_reserve if enabled; 88 bytes per step and buffer, counted in elmk_device_bytes).  elmk_run_water_balance
 * reads them as elmk_run_diagnostics reads its rows: it synchronises, copies the rows of the most recently enqueued run (any pointer
 * may be NULL) and returns their number, 0 if that run did not carry the flag.  The run is refused before anything is enqueued when
 * the feature is not enabled or the flag comes without ELMK_RUN_HYDROLOGY.  Graph on and off give the same bits.
 * The rows are recomputed every step and are not part of restart images.  A context that never enables the feature runs the kernels,
 * launch sequences and graphs it ran before, allocates nothing more and saves the image it saved before. */
enum { ELMK_WB_BEGWB = 0, ELMK_WB_ERRH2O = 1, ELMK_WB_QRUNOFF = 2, ELMK_WB_ENDWB = 3, ELMK_WB_SOILWATER_10CM = 4, ELMK_WB_TOTSOILLIQ = 5,
       ELMK_WB_TOTSOILICE = 6, ELMK_WB_NROWS = 7 };
#define ELMK_RUN_WATER_BALANCE 64 /* the seventh flag bit of elmk_run: every step closes the water budget */
int elmk_water_balance_enable(elmk_ctx *ctx, double tol_mm);
int elmk_water_balance_begin(elmk_ctx *ctx);
int elmk_water_balance(elmk_ctx *ctx, double dt, double *min_max_sum /*[3][3] or NULL*/, int64_t *nbad, int64_t *first_bad_col);
int elmk_water_balance_read(elmk_ctx *ctx, int which, double *host, int64_t col0, int64_t n);
int elmk_water_balance_clear(elmk_ctx *ctx);
int elmk_run_water_balance(elmk_ctx *ctx, double *min_max_sum /*[nsteps][3][3]*/, int64_t *nbad /*[nsteps]*/, int64_t *first_bad_col /*[nsteps]*/);

/* ---- irrigation ------------------------------------------------------------------------------------
 * ELM's irrigation (CLM4.5 / ELM v1): the daily demand check of CanopyFluxes and the application of canopy_hydrology's Irrigation()
 * and ground_flux.  The reference carries the three names and hardwires them: irrig_rate = 0.0 and n_irrig_steps_left = 0
 * (driver/kokkos/elm_kokkos_interface.cc:98-99), qflx_irrig = 0.0 (driver/kokkos/canopy_hydrology_kokkos.cc:24); Irrigation()
 * (src/physics/canopy_hydrology_impl.hh:70-80) is never called and the routine that sets the rate is a comment block
 * (src/physics/canopy_fluxes_impl.hh:17-91).  This opt-in stage is both, one launch between the seven wrappers and soil_temperature:
 * the two fields it changes, qflx_rain_grnd and qflx_snwcp_liq, are stored by canopy_hydrology and read by nothing before
 * snow_hydrology and surface_fluxes.  elmkernels_amd/irrigation.py: step() is the same operation on the host.
 *
 * The feature owns three fp64 rows [level stride] (in both builds): ELMK_IRR_RATE = irrig_rate (mm/s), ELMK_IRR_NLEFT =
 * n_irrig_steps_left (a small whole number, exact in fp64, so that the row read, history row entries and restart sections serve it
 * unchanged), ELMK_IRR_QFLX_IRRIG = this step's applied rate (mm/s; a diagnostic, overwritten every step); and one int32 parameter row
 * sched[c]: -1 = the column is not irrigated, else the column's longitude offset in seconds, 0 .. 86399 (irrigation.schedule:
 * ELM's round(londeg / degpsec), degpsec = 15 / 3600, half away from zero, reduced mod 86400).  Which columns are irrigated is the
 * driver's surface data, like hksat.
 *
 * One step, per column c.  idt = the step length in whole seconds, dt = idt as a double, tod = seconds after midnight UTC at the start
 * of the step (0 .. 86399), nspd = (14400 + (idt - 1)) / idt (integer division: the steps of the four-hour window).  Conventions of
 * "soil hydrology": no contraction, plain IEEE comparisons, `/` the correctly rounded division, pow is glibc's (elmk_pow),
 * max(a, b) = (a < b ? b : a), state fields widened to fp64 as stored; a NaN stored into a row is the canonical quiet NaN.
 * Soil layer j = 0 .. 14 is level 5 + j of t_soisno, h2osoi_liq and dz and level j of rootfr, eff_porosity, sucsat and bsw;
 * denh2o = 1000, tfrz = 273.15; smpso is the PFT parameter of the column's vtype, as calc_root_moist_stress reads it.
 * A (apply: Irrigation(), then ground_flux's qflx_prec_grnd_rain + qflx_irrig):
 *   n = NLEFT[c];  if (n > 0) { q = RATE[c];  NLEFT[c] = n - 1; } else q = +0.0;
 *   QFLX_IRRIG[c] = q;
 *   if (q > 0.0) { if (do_capsnow[c]) qflx_snwcp_liq[c] += q;  else qflx_rain_grnd[c] += q; }    (added and rounded at state precision)
 *   In the fp64 build this is bit for bit the reference's sum: the stored field is prec_rain + 0.0, which differs from prec_rain only
 *   where prec_rain is -0.0, and there both sums equal q.
 * B (check, after A in the same thread - ELM's order: hydrology before fluxes, the new rate serves the following steps):
 *   if (sched[c] >= 0 && frac_veg_nosno[c] != 0 && elai[c] > 0.0 && btran[c] < 0.999999) {
 *     local = (tod + sched[c]) % 86400;  since = (local - 21600 + 86400) % 86400;
 *     if (since < idt) {                                   (the step in which the local clock passes 06:00)
 *       NLEFT[c] = nspd;  rate = +0.0;
 *       for j = 0 .. 14:
 *         if (t_soisno[j] <= tfrz) break;                  (no layer below a frozen one is measured)
 *         if (rootfr[j] > 0.0) {
 *           vol_liq_so = eff_porosity[j] * pow(-smpso / sucsat[j], -1.0 / bsw[j]);
 *           liq_so = vol_liq_so * denh2o * dz[j];  liq_sat = eff_porosity[j] * denh2o * dz[j];
 *           deficit = max((liq_so + 0.7 * (liq_sat - liq_so)) - h2osoi_liq[j], 0.0);
 *           rate = rate + deficit / (dt * nspd); }
 *       RATE[c] = rate; } }
 * btran and eff_porosity are this step's: both elmk_timestep7 and elmk_timestep7_fused leave them in the state.
 * The integer fields are read by C's rules: any non-zero frac_veg_nosno (-1 and 2 as well as 1) counts as vegetated and any non-zero
 * do_capsnow as capped.  The clock is read at the step's start: a column checks in the step that starts less than idt seconds after
 * its local 06:00:00 (since = 0 .. idt - 1), so a step of 86400 s checks every eligible column.
 *
 *   elmk_irrigation_enable  allocates the rows and sched (3 x 8 + 4 bytes x elmk_level_stride in one owner, counted in
 *                           elmk_device_bytes), the rows zero-filled; drops the captured run step.  ELMK_E_INVALID, nothing changed:
 *                           already enabled; a null sched; a sched value outside -1 .. 86399; a stream being captured.
 *   elmk_irrigation_init    RATE and NLEFT from host[ncols] each (NULL: zeros), QFLX_IRRIG = zeros.  Synchronises.  ELMK_E_INVALID,
 *                           nothing changed: not enabled; a rate that is not finite or negative; an nleft that is not a whole number
 *                           in 0 .. 86400; a stream being captured.
 *   elmk_irrigation         one launch; stream-ordered and capturable, no host memory, no synchronisation.  ELMK_E_INVALID, nothing
 *                           enqueued: not enabled; dt not a finite whole number of seconds in 1 .. 86400; tod_seconds outside
 *                           0 .. 86399.  A context whose land unit (elmk_set_land) is not soil or crop enqueues nothing and returns
 *                           ELMK_OK (the reference's !lakpoi && !urbpoi).
 *   elmk_irrigation_read    row `which` (ELMK_IRR_*) of columns [col0, col0 + n) as doubles; synchronises.
 *   elmk_irrigation_clear   frees the rows and sched and drops the captured run step; refused while a history row entry of the family
 *                           exists ("elmk_history_clear first").
 * Stepwise placement: elmk_timestep7_fused (or elmk_timestep7), elmk_irrigation, elmk_soil_temperature, elmk_snow_hydrology,
 * elmk_surface_fluxes.  elmk_advance_physics stays exactly what it is and never irrigates.
 * elmk_run with ELMK_RUN_IRRIGATION runs the stage in every step between the last fused group and soil_temperature, with
 * tod = llround((decday - 1.0 - doy) * 86400.0) reduced to 0 .. 86399, derived on the host from the step's start (elmk_run_step does not
 * grow); refused before anything is enqueued when the feature is not enabled or dt is not a whole number of seconds in 1 .. 86400.
 * Graph on and off give the same bits.
 * Water balance: while the feature is enabled W4 of "water balance" takes ELM's BalanceCheck form,
 *   ERRH2O = ENDWB - BEGWB - (((forc_rain + forc_snow) + QFLX_IRRIG) - QRUNOFF - qflx_evap_tot - qflx_snwcp_ice) * dt.
 * Water withdrawal: QRUNOFF stays the column's generated runoff.  With the runoff routing enabled ("runoff routing" below)
 * elmk_routing_set_withdrawal takes the applied water out of the channel storage of the column's cell; supply is not limited by that
 * storage unless the river supply limit is on ("irrigation: river supply limit" below).  Without it a driver that takes the water from the river subtracts its QIRRIG tape itself.
 * History: ELMK_ROWS_IRRIGATION (which = ELMK_IRR_*) puts ELM's QIRRIG on a tape.  Restart: a context with the feature enabled saves a
 * version-5 image that carries RATE and NLEFT ("restart" below); sched is a parameter the loading context sets itself.
 * A context that never enables the feature runs the kernels, launch sequences and graphs it ran before, allocates nothing more and
 * saves the image it saved before. */
enum { ELMK_IRR_RATE = 0, ELMK_IRR_NLEFT = 1, ELMK_IRR_QFLX_IRRIG = 2 };
#define ELMK_RUN_IRRIGATION 128 /* the eighth flag bit of elmk_run: every step applies and checks irrigation */
int elmk_irrigation_enable(elmk_ctx *ctx, const int32_t *sched /*[ncols]*/);
int elmk_irrigation_init(elmk_ctx *ctx, const double *rate /*[ncols] or NULL*/, const double *nleft /*[ncols] or NULL*/);
int elmk_irrigation(elmk_ctx *ctx, double dt, int tod_seconds);
int elmk_irrigation_read(elmk_ctx *ctx, int which, double *host, int64_t col0, int64_t n);
int elmk_irrigation_clear(elmk_ctx *ctx);

/* ---- irrigation: river supply limit ----------------------------------------------------------------
 * CLM5's and ELM's limit of the demand check by the river (limit_irrigation_if_rof_enabled, irrig_river_volume_threshold,
 * CalcDeficitVolrLimited): at the daily check the demand of a cell's columns is compared with the water the cell's channel held at the
 * end of the previous step, and if the demand is larger every demanding column of the cell is scaled back by one ratio.  Opt-in, with
 * entries of its own and no run flag: while the limit is on, elmk_irrigation and the ELMK_RUN_IRRIGATION stage of elmk_run enqueue one
 * more launch (k_irrigation_supply in k_history.hip) right behind the irrigation's on the same stream.  elmkernels_amd/irrigation.py: supply_limit()
 * is the same operation on the host.  Needs the irrigation, the runoff routing ("runoff routing" below) with the withdrawal on, and an
 * output grid in which every column lies in at most one cell.
 *
 * Conventions of "irrigation"; idt, nspd as there and dtn = (double)idt * (double)nspd.  M = the output grid's map (ptr, col, w), area
 * and VOLR the routing's, thr the threshold of elmk_irrigation_supply_enable.  The cell rows are [4][ncells rounded up to 64] fp64 in
 * both builds: ELMK_IRRSUP_DEMAND, ELMK_IRRSUP_COMMITTED (m3), ELMK_IRRSUP_RATIO (diagnostics, overwritten every step) and
 * ELMK_IRRSUP_UNMET_SUM (m3, the feature's only prognostic row).
 * S0. Column i CHECKED IN THIS STEP iff NLEFT[i] == (double)nspd after the irrigation's launch.  The marker is exact: A of "irrigation"
 *     applies (n - 1) before B checks (= nspd), in the same thread.  A column that did not take B in this launch holds either what it
 *     held before (n <= 0 unchanged, at most 0) or n - 1 of an n that an earlier B set to the nspd of its step, so at most nspd - 1
 *     while dt is unchanged; only B stores nspd.  (A driver that changes dt between steps inside an open window, or that hands
 *     elmk_irrigation_init an nleft equal to nspd, marks columns itself: the first step after either is the driver's to place.)
 *     k_irrigation is not changed.
 * S1. x[i] = RATE[i] * ((double)idt * NLEFT[i]): the depth in mm the column will still draw in its open window; for a checking column
 *     the whole new window.
 * S2. Per cell c two aggregates through M with the arithmetic of "output grid" (w[p0] * v, then + w[p] * v in CSR order, no
 *     contraction): D[c] over d[i] = x[i] for a checking column and 0.0 for every other; C[c] over c[i] = e[i] + y[i], where e[i] = x[i]
 *     for a non-checking column with NLEFT > 0 and 0.0 for every other, and y[i] = QFLX_IRRIG[i] * (double)idt is the depth the column
 *     was given in THIS step: the routing takes it out of VOLR only later in the step, so the VOLR the check sees still holds it.  A
 *     cell without terms gives 0.0 for both.
 * S3. Vd = (D * 0.001) * area[c];  Vc = (C * 0.001) * area[c]   (R1's shape);  a = VOLR[c] * (1.0 - thr) - Vc;
 *     avail = a > 0.0 ? a : 0.0   (a NaN storage supplies nothing).
 * S4. ratio = Vd > avail ? avail / Vd : 1.0.
 * S5. Every checking column of the cell: RATE[i] = RATE[i] * ratio, stored only where ratio != 1.0 (the bits are the same either way);
 *     a column in no cell is not limited; a NaN is stored as the canonical quiet NaN.
 * S6. DEMAND[c] = Vd;  COMMITTED[c] = Vc;  RATIO[c] = ratio;  UNMET_SUM[c] = UNMET_SUM[c] + (Vd - Vd * ratio).
 * Vc is not in CLM: there all columns of a gridcell share one clock.  Here sched is each column's longitude, so the columns of a cell
 * may check in adjacent steps, and without Vc the second batch would be promised water the first already holds.
 * Guaranteed: at a check, committed plus newly granted water does not exceed (1 - thr) * VOLR of the previous step's end, committed
 * being everything granted and not yet withdrawn from that VOLR (the open windows' remainders and this step's application).  Without
 * y the remainder would miss one step of every open window - NLEFT is already counted down when the limit runs - and two batches of
 * one cell in adjacent steps could be granted (1 - thr) * (1 + 1 / nspd) of the storage: more than all of it for thr = 0.1, nspd = 8.
 * Not guaranteed: the channel also releases water downstream during the four-hour window; thr is the margin for that.
 *
 *   elmk_irrigation_supply_enable  allocates the four rows, zero-filled (one owner, counted in elmk_device_bytes) and drops the captured
 *                           run step.  ELMK_E_INVALID, nothing changed: the irrigation not enabled; the routing not enabled or its
 *                           withdrawal off; threshold not finite or outside [0, 1); a column in more than one cell of the output grid
 *                           (or twice in one) - the text names the first such column; already enabled; a stream being captured.
 *   elmk_irrigation_supply_init    UNMET_SUM from host[ncells] (NULL: zeros), the other rows zeros: a restart file's values.  Synchronises.
 *   elmk_irrigation_supply_read    row `which` (ELMK_IRRSUP_*) of cells [cell0, cell0 + n) as doubles; synchronises.
 *   elmk_irrigation_supply_reset   UNMET_SUM = zeros (stream-ordered).
 *   elmk_irrigation_supply_clear   frees the rows and drops the captured run step.
 * While the limit is on what it reads stays: elmk_routing_set_withdrawal(ctx, 0), elmk_routing_clear, elmk_irrigation_clear,
 * elmk_set_output_grid and elmk_clear_output_grid are refused with ELMK_E_INVALID ("elmk_irrigation_supply_clear first") and nothing
 * changes.  elmk_routing_kinematic_enable and elmk_routing_kinematic_clear leave VOLR's buffer where it is and stay allowed.
 * A captured run step is keyed by whether the limit is on.  Restart: the rows live on cells and are not part of the column image; a
 * driver carries UNMET_SUM through elmk_irrigation_supply_read / _init, as it carries VOLR.  Multi-rank: as the routing, a context
 * limits the cells it holds completely.
 * A context that never enables the limit runs the kernels, launch sequences and graphs it ran before, allocates nothing more and saves
 * the image it saved before. */
enum { ELMK_IRRSUP_DEMAND = 0, ELMK_IRRSUP_COMMITTED = 1, ELMK_IRRSUP_RATIO = 2, ELMK_IRRSUP_UNMET_SUM = 3 };
int elmk_irrigation_supply_enable(elmk_ctx *ctx, double threshold);
int elmk_irrigation_supply_init(elmk_ctx *ctx, const double *unmet_sum /*[ncells] or NULL*/);
int elmk_irrigation_supply_read(elmk_ctx *ctx, int which, double *host, int64_t cell0, int64_t n);
int elmk_irrigation_supply_reset(elmk_ctx *ctx);
int elmk_irrigation_supply_clear(elmk_ctx *ctx);

/* ---- runoff routing --------------------------------------------------------------------------------
 * The linear-reservoir river transport model the CLM family shipped as RTM, over the output grid's cells ("output grid"): every cell
 * passes water to one downstream cell, the input is the water balance's QRUNOFF row aggregated onto the cells, and the result is the
 * channel storage and the discharge of every cell.  Routing is a recurrence in time, so a driver that wants discharge would otherwise
 * download the gridded runoff every step; this opt-in stage keeps it on the device.  k_routing.hip; elmkernels_amd/routing.py: call()
 * is the same operation on the host.  A context routes the basins whose cells it holds completely; nothing here is collective.
 *
 * Conventions of "soil hydrology": no contraction, left-associated + - *, `/` the correctly rounded fp64 division, plain IEEE
 * comparisons; every row is fp64 in both builds; a NaN stored into a row is the canonical quiet NaN.
 *
 * Network, given at enable time: ncells (the output grid's), down[ncells] (int32: the downstream cell, -1 = an outlet, ocean or
 * interior sink), ddist[ncells] (metres to the downstream cell; for an outlet the length of its own reach), area[ncells] (square metres
 * of land the cell's runoff stands for), effvel (the effective velocity in m/s, RTM's 0.35), nsub (sub-steps per call).  The host
 * derives KOUT[c] = effvel / ddist[c] (one division) and the upstream map up[8][ncells]: the cells u with down[u] == c in ascending u,
 * padded with -1; nup is the largest in-degree rounded up to 1, 2, 4 or 8 (as the forcing grid's npts).
 *
 * State and rows, each [ncells rounded up to 64] doubles: ELMK_ROUTE_VOLR (m3, the only prognostic row), ELMK_ROUTE_QIN (m3/s),
 * ELMK_ROUTE_QOUT (m3/s: the mean over the call's sub-steps of the flow leaving the cell), ELMK_ROUTE_QOUT_SUM (the sum of QOUT over
 * the calls since the last reset), and a host-side call count.
 *
 * One call elmk_routing(ctx, dt):
 * R0. dts = dt / (double)nsub.
 * R1. (once per call) r = the aggregate of the QRUNOFF row over the cell's terms, exactly the expression and order of "output grid":
 *     w[p0] * x[col[p0]], then + w[p] * x[col[p]]; a cell without terms takes r = 0.0 (not fill).  With the withdrawal on, i = the same
 *     aggregate of the irrigation's QFLX_IRRIG row and r = r - i.  QIN[c] = (r * 0.001) * area[c].
 * R2. flow(v, k): if (v > 0.0) { a = v * k;  b = v / dts;  flow = (a < b) ? a : b; } else flow = 0.0.  A NaN, zero, negative-zero or
 *     negative storage releases nothing; the cap b keeps a cell from releasing more than it holds when k * dts >= 1.
 * R3. per sub-step and cell: f = flow(v_old[c], KOUT[c]);  fin = 0.0;  for p = 0 .. 7 ascending with u = up[p][c] >= 0:
 *     fin = fin + flow(v_old[u], KOUT[u]).
 * R4. v_new[c] = v_old[c] + ((fin - f) + QIN[c]) * dts.  Every cell reads the storages of the sub-step's start (the device keeps two
 *     storage buffers and uses them in turn; the order between sub-steps is the launch boundary).
 * R5. qacc starts at 0.0 and takes qacc + f every sub-step.  After the last: QOUT = qacc / (double)nsub;  VOLR = v;
 *     QOUT_SUM = QOUT_SUM + QOUT.
 * R6. (elmk_routing_budget) sums[0] = the sum of VOLR, sums[1] = the sum of QIN, sums[2] = the sum of QOUT over the outlets, a cell that
 *     is no outlet contributing +0.0; each is the `sum` of elmk_evaluate_conservation's reduction over the cells (diagnostics.
 *     reduce_min_max_sum), bit for bit, from the same reduction kernels.
 * A call takes nsub + 1 launches (R1, then one per sub-step), each stream-ordered, host-free and capturable as one chain of nodes.
 * Supply is not limited by storage unless the irrigation's river supply limit is on ("irrigation: river supply limit" above): with the
 * withdrawal on VOLR may go negative, and a negative storage releases nothing until the inflow has refilled it.
 *
 *   elmk_routing_enable     allocates the rows, zero-filled, KOUT, area and the maps (one owner, counted in elmk_device_bytes) and
 *                           drops the captured run step.  ELMK_E_INVALID, nothing changed: no output grid; ncells other than the output
 *                           grid's; the water balance not enabled; already enabled; effvel not finite and > 0; nsub outside 1 .. 64; a
 *                           null array; a down outside [-1, ncells) or equal to its own index; more than 8 upstream cells draining into
 *                           one cell; a cycle; a ddist that is not finite and > 0; an area that is not finite and >= 0; a stream being
 *                           captured.
 *   elmk_routing_init       VOLR and QOUT_SUM from host[ncells] each (NULL: zeros), QIN and QOUT zeros, the call count = ncalls >= 0: a
 *                           restart file's values.  Synchronises.
 *   elmk_routing            one call; stream-ordered and capturable, no host memory, no synchronisation; the call count advances by one.
 *                           ELMK_E_INVALID, nothing enqueued: not enabled; dt not finite and positive.
 *   elmk_routing_read       row `which` (ELMK_ROUTE_*) of cells [cell0, cell0 + n) as doubles; synchronises.
 *   elmk_routing_count      the calls since the last elmk_routing_init / elmk_routing_reset_mean: QOUT_SUM / count is the mean discharge.
 *   elmk_routing_reset_mean QOUT_SUM = zeros (stream-ordered), the count = 0.
 *   elmk_routing_set_withdrawal  on != 0: R1 subtracts the irrigation's applied water; refused without the irrigation enabled.  Off
 *                           (the default) gives the bits of a context that never called it.
 *   elmk_routing_budget     R6; synchronises.
 *   elmk_routing_clear      frees everything and drops the captured run step.
 * While the feature is enabled what it reads stays: elmk_set_output_grid, elmk_clear_output_grid, elmk_water_balance_clear,
 * elmk_soil_hydrology_clear and, with the withdrawal on, elmk_irrigation_clear are refused with ELMK_E_INVALID ("elmk_routing_clear
 * first") and nothing changes.
 * elmk_run with ELMK_RUN_ROUTING runs the call in every step with the run's dt, after W1 - W8 of the water balance and before the
 * active layer update, the accumulated fields and the history; refused before anything is enqueued when the feature is not enabled or
 * the flag comes without ELMK_RUN_WATER_BALANCE.  The call count advances by nsteps at enqueue.  Graph on and off give the same bits.
 * Restart: the routing state lives on cells and is not part of the column image ("restart").  A driver saves VOLR, QOUT_SUM and the
 * count with elmk_routing_read / elmk_routing_count and restores them with elmk_routing_init after elmk_routing_enable.
 * A context that never enables the feature runs the kernels, launch sequences and graphs it ran before, allocates nothing more and
 * saves the image it saved before. */
enum { ELMK_ROUTE_VOLR = 0, ELMK_ROUTE_QIN = 1, ELMK_ROUTE_QOUT = 2, ELMK_ROUTE_QOUT_SUM = 3 };
#define ELMK_RUN_ROUTING 256 /* the ninth flag bit of elmk_run: every step routes the step's runoff */
int elmk_routing_enable(elmk_ctx *ctx, int64_t ncells, const int32_t *down, const double *ddist, const double *area, double effvel, int nsub);
int elmk_routing_init(elmk_ctx *ctx, const double *volr /*[ncells] or NULL*/, const double *qout_sum /*[ncells] or NULL*/, int64_t ncalls);
int elmk_routing(elmk_ctx *ctx, double dt);
int elmk_routing_read(elmk_ctx *ctx, int which, double *host, int64_t cell0, int64_t n);
int elmk_routing_count(elmk_ctx *ctx, int64_t *ncalls);
int elmk_routing_reset_mean(elmk_ctx *ctx);
int elmk_routing_set_withdrawal(elmk_ctx *ctx, int on);
int elmk_routing_budget(elmk_ctx *ctx, double *sums /*[3]*/);
int elmk_routing_clear(elmk_ctx *ctx);

/* ---- kinematic-wave routing ------------------------------------------------------------------------
 * An opt-in second scheme of the routing stage above, after the river model the E3SM land model routes with today (MOSART): runoff
 * passes through three stores per cell - the hillslope (overland flow), the sub-network of tributaries and the main channel - and each
 * releases by Manning's equation, so the velocity rises with the hydraulic radius.  Surface runoff enters the hillslope, subsurface
 * runoff the tributaries.  The statement below is the specification; k_routing.hip (k_kinematic_prep, k_kinematic_step) performs it
 * and elmkernels_amd/routing.py: kinematic_call() restates it on the host.
 *
 * Conventions of "runoff routing": no contraction, left-associated + - *, `/` the correctly rounded fp64 division, sqrt correctly
 * rounded, plain IEEE comparisons; every row is fp64 in both builds; a NaN is stored as the canonical quiet NaN.  pow is elmk_pow on the
 * device (elmk_math.h: glibc's bits) and glibc's pow on the host.  T23 = 2.0 / 3.0 and T53 = 5.0 / 3.0 are the doubles those quotients
 * give.
 *
 * Parameters, given once after elmk_routing_enable as params[ELMK_KW_NPARAM][ncells]: HSLP (hillslope slope), NH (hillslope Manning
 * n), GXR (drainage density, 1/m), TLEN, TWIDTH (tributary length and width, m), TSLP, NT (tributary slope and Manning n), RLEN, RWIDTH
 * (main channel length and width, m), RSLP, NR (main channel slope and Manning n).  Every value must be finite and > 0.  The host
 * derives CH = (sqrt(HSLP) / NH) * GXR, CT = sqrt(TSLP) / NT, CR = sqrt(RSLP) / NR and keeps CH, CT, CR, TLEN, TWIDTH, RLEN, RWIDTH on
 * the device.  effvel, ddist and KOUT are not read while the scheme is on; area, down, the upstream map, nsub and the withdrawal
 * switch stay the routing's.
 *
 * State and rows: ELMK_ROUTE_VOLR is the main channel's storage (m3) while the scheme is on; new prognostic rows ELMK_ROUTE_WH
 * (hillslope water, m3) and ELMK_ROUTE_WT (tributary storage, m3); new diagnostic row ELMK_ROUTE_QSUR (m3/s: the surface part of
 * QIN).  QIN, QOUT and QOUT_SUM keep their meaning.  elmk_routing_read accepts the three new rows only while the scheme is on.
 *
 * One call elmk_routing(ctx, dt) while the scheme is on:
 * K0. dts = dt / (double)nsub.
 * K1. (once per call) QIN exactly as R1, withdrawal included.  s = the aggregate over the cell's terms, in R1's order, of
 *     w[p] * (QFLX_SURF[col[p]] + QFLX_H2OSFC_SURF[col[p]]), the soil hydrology's rows; a cell without terms takes 0.0.
 *     QSUR = (s * 0.001) * area;  QSUB = QIN - QSUR.
 * K2. cap(v, a): if (v > 0.0) { b = v / dts;  cap = (a < b) ? a : b; } else cap = 0.0.  R2 with the rate already formed.
 * K3. hillslope: if (area > 0.0) { h = WH / area;  eh = cap(WH, (CH * pow(h, T53)) * area); } else eh = 0.0.
 * K4. chan(w, len, wid, c): a = w / len;  y = a / wid;  p = wid + 2.0 * y;  r = a / p;  chan = cap(w, (c * pow(r, T23)) * a).
 *     et = chan(WT, TLEN, TWIDTH, CT);  er = chan(VOLR, RLEN, RWIDTH, CR).
 * K5. fin = 0.0; for p = 0 .. 7 ascending with u = up[p][c] >= 0: fin = fin + er[u], the upstream cell's er of this sub-step's start.
 * K6. all three flows are evaluated from the storages of the sub-step's start; then WH = WH + (QSUR - eh) * dts;
 *     WT = WT + ((eh - et) + QSUB) * dts;  VOLR = VOLR + ((fin - er) + et) * dts.
 * K7. qacc starts at 0.0 and takes qacc + er every sub-step.  After the last: QOUT = qacc / (double)nsub;
 *     QOUT_SUM = QOUT_SUM + QOUT.
 * K8. (elmk_routing_kinematic_budget) sums[0] = the sum of WH, sums[1] = the sum of WT, through the reduction kernels of R6.  With
 *     elmk_routing_budget's three sums: the change of (sum WH + sum WT + sum VOLR) over a call = dt (sum QIN - sum outlet QOUT).
 * K9. A NaN, zero, negative or -inf storage releases nothing, as in R2 (where the cap returns 0.0 the rate is not formed).
 * A call takes nsub + 1 launches, as the linear scheme's.  The device keeps a row of er per cell in two buffers: the K1 launch writes
 * the er of the call's first sub-step, every sub-step but the last writes the er of its new VOLR for the next to gather (the same
 * operands through the same operations as evaluating it there), and WH, WT and VOLR update in place.
 *
 *   elmk_routing_kinematic_enable  takes the parameters, allocates the scheme's rows zero-filled (one owner, counted in
 *                           elmk_device_bytes) and drops the captured run step.  ELMK_E_INVALID, nothing changed: the routing not
 *                           enabled; the soil hydrology not enabled; already on; a null argument; a value that is not finite and > 0
 *                           (the text names the row, "elmk_routing_kinematic_enable: TLEN not finite and > 0"); a stream being captured.
 *   elmk_routing_kinematic_init    WH and WT from host[ncells] each (NULL: zeros), QSUR zeros.  VOLR, QOUT_SUM and the count stay
 *                           elmk_routing_init's.  Synchronises.
 *   elmk_routing_kinematic_budget  K8; synchronises.
 *   elmk_routing_kinematic_clear   back to the linear scheme with VOLR, QOUT_SUM and the count kept; frees what enable allocated and
 *                           drops the captured run step.  elmk_routing_clear frees both.
 * elmk_routing and elmk_run with ELMK_RUN_ROUTING run whichever scheme is on; the call count and elmk_routing_reset_mean are unchanged.
 * Restart: a driver saves WH and WT with elmk_routing_read beside VOLR, QOUT_SUM and the count and restores them with
 * elmk_routing_kinematic_init after elmk_routing_kinematic_enable.  A context that never calls these entries runs the kernels, launch
 * sequences and graphs it ran before and allocates nothing more. */
enum { ELMK_ROUTE_WH = 4, ELMK_ROUTE_WT = 5, ELMK_ROUTE_QSUR = 6 };
enum {
  ELMK_KW_HSLP = 0, ELMK_KW_NH = 1, ELMK_KW_GXR = 2, ELMK_KW_TLEN = 3, ELMK_KW_TWIDTH = 4, ELMK_KW_TSLP = 5, ELMK_KW_NT = 6,
  ELMK_KW_RLEN = 7, ELMK_KW_RWIDTH = 8, ELMK_KW_RSLP = 9, ELMK_KW_NR = 10, ELMK_KW_NPARAM = 11
};
int elmk_routing_kinematic_enable(elmk_ctx *ctx, const double *params /*[ELMK_KW_NPARAM][ncells]*/);
int elmk_routing_kinematic_init(elmk_ctx *ctx, const double *wh /*[ncells] or NULL*/, const double *wt /*[ncells] or NULL*/);
int elmk_routing_kinematic_budget(elmk_ctx *ctx, double *sums /*[2]*/);
int elmk_routing_kinematic_clear(elmk_ctx *ctx);

/* ---- floodplain inundation ----------------------------------------------------------------------
 * An opt-in extension of the kinematic-wave scheme above, after MOSART-Inundation (Luo et al., Geosci. Model Dev. 10, 2017): the main
 * channel gets banks.  The channel holds RLEN * RWIDTH * RDEPTH; what exceeds that spreads over a floodplain described by an elevation
 * profile, channel and floodplain share one water level, and only the water over the channel bed flows downstream (K4 reads the
 * channel's share), so a flood wave is held back instead of running ever faster.  The pattern is the frost table's: a template
 * parameter on the existing kernel (k_routing.hip: k_kinematic_step<.., FLOOD>), no run flag and no new call in the step.
 * elmkernels_amd/routing.py: inundation_tables(), inundation_exchange() and kinematic_call(..., flood=) restate it on the host.
 *
 * Conventions of "kinematic-wave routing": no contraction, left-associated + - *, `/` and sqrt correctly rounded, plain IEEE
 * comparisons, every row fp64 in both builds, a NaN stored as the canonical quiet NaN.
 *
 * Inputs, given once after elmk_routing_kinematic_enable: rdepth[ncells], the bank height in metres, finite and > 0; and
 * eprof[ELMK_FP_NPROF][ncells], E_k = eprof[k][c] the elevation above the bank top at which the fraction k / 10 of the floodplain is
 * wet: finite, E_0 == 0.0, strictly increasing in k.
 *
 * Rows: ELMK_ROUTE_WF (m3, the floodplain storage; the extension's only prognostic row), ELMK_ROUTE_FLOOD_DEPTH (m above the bank
 * top) and ELMK_ROUTE_FLOOD_FRAC (the share of the cell's area under floodplain water), two diagnostics that hold the value of the
 * call's last sub-step.  elmk_routing_read accepts the three only while the extension is on.
 *
 * I0. host tables, once, in this order: ACHN = RLEN * RWIDTH;  VC = ACHN * RDEPTH;  AF = area - ACHN, taken as 0.0 unless > 0.0;
 *     f_k = (double)k / 10.0;  S_k = ACHN + AF * f_k;  DE_k = E_{k+1} - E_k;  M_k = (AF * 0.1) / DE_k;  VB_0 = 0.0;
 *     VB_{k+1} = VB_k + (0.5 * (S_k + S_{k+1})) * DE_k.  S_k is the wet surface at level E_k (channel included), M_k its growth per
 *     metre inside segment k, VB_k the volume over the bank top at level E_k.
 * I1. The exchange runs per sub-step and cell after K6 has formed the new VOLR v, before that VOLR is stored and before the next
 *     sub-step's er is formed from it.  If !(WF > 0.0 || v > VC) nothing is touched: VOLR, WH, WT, er and QOUT keep the bits of the
 *     plain scheme, and FLOOD_DEPTH = FLOOD_FRAC = 0.0.
 * I2. W = v + WF.  If !(W > VC): VOLR = W;  WF = 0.0;  both diagnostics 0.0.  The floodplain drains back at once; a NaN W takes
 *     this path.
 * I3. Otherwise X = W - VC.  If X >= VB_10: h = E_10 + (X - VB_10) / S_10 and f = 1.0.  Else with k the largest of 0 .. 9 with
 *     X >= VB_k:  r = X - VB_k;  d = (2.0 * r) / (S_k + sqrt(S_k * S_k + (2.0 * M_k) * r));  if (d > DE_k) d = DE_k;  h = E_k + d;
 *     f = f_k + (0.1 * d) / DE_k.  (d solves S_k d + M_k d^2 / 2 = r in the form that does not cancel.  h and f rise with W up to
 *     their own rounding: between neighbouring doubles h may step back by an ulp, and where d reaches DE_k the sum f_k + 0.1 may lie
 *     an ulp or two above f_{k+1}, as 0.2 + 0.1 does.)
 * I4. vc2 = VC + ACHN * h;  if (vc2 > W) vc2 = W.  VOLR = vc2;  WF = W - vc2;  FLOOD_DEPTH = h;
 *     FLOOD_FRAC = (area > 0.0) ? (AF * f) / area : 0.0.
 * I5. K4 is unchanged: er is evaluated from the post-exchange VOLR, so the water column over the channel moves and the floodplain
 *     stands still.
 * I6. The K1 launch does no exchange: the first sub-step's er comes from VOLR as the last call or elmk_routing_init left it.
 * I7. (elmk_routing_inundation_budget) sums[0] = the sum of WF through R6's reduction kernels.  The change of
 *     sum WH + sum WT + sum VOLR + sum WF over a call = dt (sum QIN - sum outlet QOUT).
 * I8. Edge values do what I1 - I4 say literally.  A NaN, zero or negative WF with v <= VC, or a NaN v with such a WF, is untouched
 *     (I1); a NaN v with WF > 0.0, or a NaN WF with v > VC, gives W = NaN: VOLR = NaN, WF = 0.0 (I2); a negative WF with v > VC is
 *     added like any other; W = +inf gives h = +inf, VOLR = +inf and WF = inf - inf = NaN; -inf never passes I1 or takes I2.
 * The device keeps VC, ACHN, AF, E and VB as rows and forms S_k, DE_k and M_k again with I0's operations (the same bits); a cell that
 * passes I1 untouched reads VC and WF and nothing else of them.
 *
 *   elmk_routing_inundation_enable  takes the inputs, builds I0's tables, allocates them and the three rows zero-filled (one owner,
 *                           counted in elmk_device_bytes) and drops the captured run step.  ELMK_E_INVALID, nothing changed: the
 *                           kinematic scheme not on; already on; a null argument; a bad value (the text names the row and the first
 *                           offending cell, "elmk_routing_inundation_enable: EPROF not increasing at cell 17"); a stream being captured.
 *   elmk_routing_inundation_init    WF from host[ncells] (NULL: zeros), the diagnostics zeros.  Synchronises.
 *   elmk_routing_inundation_budget  I7; synchronises.
 *   elmk_routing_inundation_clear   back to the channel without banks, WF dropped, VOLR kept; frees what enable allocated and drops
 *                           the captured run step.  From then on the kinematic rows take the bits of a context that never had the
 *                           extension, given the same VOLR.
 * While the extension is on elmk_routing_kinematic_clear is refused with ELMK_E_INVALID ("elmk_routing_inundation_clear first");
 * elmk_routing_clear frees everything.  elmk_routing and elmk_run with ELMK_RUN_ROUTING run the flood form while it is on.  The
 * irrigation's river supply limit keeps reading VOLR: floodplain water is not available to irrigation.
 * Restart: a driver saves WF with elmk_routing_read beside VOLR, WH and WT and hands it to elmk_routing_inundation_init after
 * elmk_routing_inundation_enable; the diagnostics are rewritten by the next call.  A context that never calls these entries runs the
 * kernels, launch sequences and graphs it ran before and allocates nothing more. */
enum { ELMK_ROUTE_WF = 7, ELMK_ROUTE_FLOOD_DEPTH = 8, ELMK_ROUTE_FLOOD_FRAC = 9 };
#define ELMK_FP_NPROF 11
int elmk_routing_inundation_enable(elmk_ctx *ctx, const double *rdepth /*[ncells]*/, const double *eprof /*[ELMK_FP_NPROF][ncells]*/);
int elmk_routing_inundation_init(elmk_ctx *ctx, const double *wf /*[ncells] or NULL: zeros*/);
int elmk_routing_inundation_budget(elmk_ctx *ctx, double *sums /*[1]: the sum of WF, through R6's reduction kernels*/);
int elmk_routing_inundation_clear(elmk_ctx *ctx);

/* ---- reservoirs ---------------------------------------------------------------------------------
 * An opt-in extension of the kinematic-wave scheme above, after the water management of MOSART-WM (Voisin et al., Hydrol. Earth Syst.
 * Sci. 17, 2013; the release rules of Hanasaki et al., J. Hydrol. 327, 2006): a dam at the outlet of a cell stores water behind it
 * and releases it towards a monthly target, so the discharge below it is the regulated one, and the cell's irrigation draws on the
 * stored water.  The pattern is the inundation's: a template parameter on the existing kernels (k_routing.hip:
 * k_kinematic_prep<.., DAM>, k_kinematic_step<.., DAM>), no run flag and no new call or launch in the step.
 * elmkernels_amd/routing.py: reservoir_tables(), reservoir_prep(), reservoir_regulate() and kinematic_call(..., dam=) restate it on
 * the host.
 *
 * Conventions of "kinematic-wave routing": no contraction, left-associated + - *, `/` correctly rounded, plain IEEE comparisons, every
 * row fp64 in both builds, a NaN stored as the canonical quiet NaN.
 *
 * Inputs, given once after elmk_routing_kinematic_enable: cap[ncells], the storage capacity in m3, finite and >= 0, 0.0 = no dam;
 * target[12][ncells], the monthly target release in m3/s, finite and >= 0; beta[ncells] in [0, 1], the weight of the target against
 * the inflow; mstart[ncells], int32 in 0 .. 11, the first month of the dam's operational year.  target, beta and mstart are checked
 * only where cap > 0.0.  The host derives SMIN = 0.1 * CAP and C85 = 0.85 * CAP and keeps CAP, SMIN, C85, TARGET, BETA and MSTART on
 * the device.  elmkernels_amd/routing.py: reservoir_targets() forms target, beta and mstart from a climatology by Hanasaki's rules.
 *
 * Time: the month m (0 .. 11) and a bool `begins` (this call is the one whose step starts at 00:00 of the first day of month m) are
 * the driver's, like the active layer's rollover.  Stepwise, elmk_routing_reservoir_time(ctx, month, begins) sets what the following
 * elmk_routing calls use (0, false after the enable).  In elmk_run the host derives both from the step's doy and decday in the
 * reference's no-leap calendar - m from doy, begins = (decday == doy + 1.0) on the first doy of a month, the rollover's test - and
 * packs them into the run row's pad word above the irrigation's time of day; elmk_run_step does not grow.
 *
 * Rows: ELMK_ROUTE_RES (m3, the reservoir storage; prognostic), ELMK_ROUTE_KRLS (the release coefficient; prognostic, 1.0 after the
 * enable and after an _init without a row) and ELMK_ROUTE_RES_TAKE (m3 taken for irrigation in this call; diagnostic).
 * elmk_routing_read accepts the three only while the extension is on.
 *
 * D0. A cell is a dam cell iff CAP > 0.0.  In any other cell every row of the scheme keeps the bits of the form without the
 *     extension, and RES, KRLS and RES_TAKE are not written.  The rest of the statement is about dam cells.
 * D1. (K1 launch, once per call) if (begins && m == MSTART) KRLS = RES / C85.
 * D2. (K1 launch, only with the routing's withdrawal on) with rn and i R1's aggregates of QRUNOFF and QFLX_IRRIG:
 *     iv = (i * 0.001) * area;  want = iv * dt;  a = RES - SMIN;  avail = a > 0.0 ? a : 0.0;  t = want > avail ? avail : want;
 *     RES = RES - t;  RES_TAKE = t;  QIN = (rn * 0.001) * area - (iv - t / dt).  The dam covers what it can of the cell's
 *     withdrawal; the rest leaves the channel as in R1.  Without the withdrawal RES_TAKE = 0.0 and QIN is K1's.
 *     QSUB = QIN - QSUR, as in K1.
 * D3. (regulation) wherever K4 forms the main channel's er for a coming sub-step - the K1 launch and every sub-step but the last,
 *     in the flood form after I1 - I5 - with e that er:
 *     q = BETA * (KRLS * TARGET[m]) + (1.0 - BETA) * e;  qmin = 0.1 * e;  if (q < qmin) q = qmin;
 *     if (q > e) { a = RES - SMIN;  x = q - e;  lim = a > 0.0 ? a / dts : 0.0;  if (x > lim) x = lim;  eo = e + x; } else eo = q;
 *     s = RES + (e - eo) * dts;  if (s > CAP) { eo = eo + (s - CAP) / dts;  s = CAP; }  RES = s.
 *     The dam releases the blend of its target and its inflow, never less than a tenth of the inflow; what it releases beyond the
 *     inflow it draws from the storage above SMIN, what it holds back it stores, and what does not fit spills.
 * D4. The flow row's buffer takes eo: downstream cells' K5 and the cell's own K7 read that, so QOUT is the regulated discharge.
 *     The cell's own K6 of the coming sub-step subtracts the natural e: VOLR = VOLR + ((fin - e) + et) * dts.
 * D5. RES therefore stands one sub-step ahead of VOLR inside a call, and level with it at the call's end, because the last sub-step
 *     forms no flow.
 * D6. (elmk_routing_reservoir_budget) sums[0] = the sum of RES, sums[1] = the sum of RES_TAKE, through R6's reduction kernels.  The
 *     change of sum WH + sum WT + sum VOLR (+ sum WF) + sum RES over a call = dt (sum QIN - sum outlet QOUT) - sum RES_TAKE.
 * D7. (river supply limit) While the reservoirs and elmk_irrigation_supply_* are both on, S3 reads for a dam cell r = RES - SMIN, taken
 *     as 0.0 unless > 0.0, and a = (VOLR * (1.0 - thr) + r) - Vc.  Every other cell, and every cell with the extension off, keeps S3
 *     (k_irrigation_supply's DAM form; elmkernels_amd/irrigation.py: supply_limit(dam=)).  A NaN RES counts as nothing.
 * D8. Edge values do what D1 - D3 say literally.  A NaN RES gives a = NaN, so avail = 0.0 and lim = 0.0: nothing is taken for a positive
 *     want and nothing is drawn; s = NaN fails s > CAP and RES stays NaN, while eo is e (where q > e) or q.  A NaN KRLS or e makes q
 *     NaN, which fails both q < qmin and q > e: eo = NaN and RES = NaN.  RES = +inf has lim = +inf: a finite q draws x = q - e, and
 *     s = +inf spills: eo = +inf, RES = CAP; in a call that D1 opens, KRLS = +inf makes q and eo +inf and s = inf - inf = NaN.  A
 *     negative RES, or any RES <= SMIN, draws nothing: the dam passes e, or stores where q < e.  RES = -inf stays -inf (and D1's
 *     KRLS = -inf gives q = -inf, floored to 0.1 e).  e = +inf gives q = +inf where BETA < 1.0 (eo = q, s = RES + NaN = NaN); at
 *     BETA == 1.0 the term 0.0 * inf is NaN.  CAP = 5e-324 is a dam: SMIN = 0.0 (0.1 of the smallest double rounds to zero) and
 *     C85 = 5e-324 (0.85 of it rounds to itself), so D1 gives KRLS = +inf for any RES that is not tiny, and the reservoir draws all it
 *     holds and spills whatever it would store.
 * The device keeps the natural e of a dam cell's coming sub-step in a row of its own, which only the cell's own thread writes and
 * reads; evaluating K4 again from the VOLR of the sub-step's start would give the same operands through the same operations.
 *
 *   elmk_routing_reservoir_enable  takes the inputs, builds the tables, allocates them and the rows (RES, RES_TAKE zero-filled, KRLS
 *                           1.0; one owner, counted in elmk_device_bytes) and drops the captured run step.  ELMK_E_INVALID, nothing
 *                           changed: the kinematic scheme not on; already on; a null argument; a bad value
 *                           (the text names the row and the first offending cell, "elmk_routing_reservoir_enable: BETA outside
 *                           [0, 1] at cell 17"); a stream being captured.
 *   elmk_routing_reservoir_init    RES from host[ncells] (NULL: zeros), KRLS from host[ncells] (NULL: 1.0), RES_TAKE zeros.
 *                           Synchronises.
 *   elmk_routing_reservoir_time    the month and `begins` of the following elmk_routing calls.  ELMK_E_INVALID: month outside 0 .. 11.
 *   elmk_routing_reservoir_budget  D6; synchronises.
 *   elmk_routing_reservoir_clear   back to the free-flowing channel, RES dropped, VOLR kept; frees what enable allocated and drops the
 *                           captured run step.  From then on the scheme's rows take the bits of a context that never had the
 *                           extension, given the same VOLR.
 * While the extension is on elmk_routing_kinematic_clear is refused with ELMK_E_INVALID ("elmk_routing_reservoir_clear first");
 * elmk_routing_clear frees everything.  The reservoirs and the inundation may be enabled in either order and cleared independently.
 * elmk_routing and elmk_run with ELMK_RUN_ROUTING run the DAM form while it is on.
 * Tapes: elmk_cell_history_add_row(ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_RES | KRLS | RES_TAKE) works while the extension is on, and while
 * such an entry exists elmk_routing_reservoir_clear is refused ("elmk_history_clear first").
 * Restart: under ELMK_OPT_RESTART_CELLS a context with the reservoirs on saves an image of version 7
 * (ELMK_RESTART_VERSION_RESERVOIR): version 6 plus the cell sections ELMK_ROUTE_RES and ELMK_ROUTE_KRLS after WF; it loads only into a
 * context with the same stages on, and the load leaves RES_TAKE zero; every other context saves byte for byte what it saved before.
 * With the option off a driver saves RES and KRLS with elmk_routing_read beside the scheme's rows and hands them to
 * elmk_routing_reservoir_init after elmk_routing_reservoir_enable.  A context that never calls these entries runs the kernels,
 * launch sequences and graphs it ran before and allocates nothing more. */
enum { ELMK_ROUTE_RES = 10, ELMK_ROUTE_KRLS = 11, ELMK_ROUTE_RES_TAKE = 12 };
int elmk_routing_reservoir_enable(elmk_ctx *ctx, const double *cap /*[ncells]*/, const double *target /*[12][ncells]*/,
                                  const double *beta /*[ncells]*/, const int32_t *mstart /*[ncells]*/);
int elmk_routing_reservoir_init(elmk_ctx *ctx, const double *res /*[ncells] or NULL: zeros*/, const double *krls /*[ncells] or NULL: 1.0*/);
int elmk_routing_reservoir_time(elmk_ctx *ctx, int month /*0 .. 11*/, int begins);
int elmk_routing_reservoir_budget(elmk_ctx *ctx, double *sums /*[2]: the sums of RES and RES_TAKE, through R6's reduction kernels*/);
int elmk_routing_reservoir_clear(elmk_ctx *ctx);

/* ---- stream temperature -------------------------------------------------------------------------
 * An opt-in extension of the kinematic-wave scheme above, after the heat module of ELM's river model, MOSART-heat (Li et al., J. Adv.
 * Model. Earth Syst. 7, 2015): the tributary store and the main channel of every cell carry a water temperature, TT and TR.  Heat
 * enters with the runoff (surface runoff at the ground's temperature, subsurface runoff at a soil layer's), moves with the water,
 * and is exchanged through the water surface: absorbed shortwave and longwave, emitted longwave, sensible and latent heat.  The
 * pattern is the inundation's and the reservoirs': a template parameter on the existing kernels (k_routing.hip:
 * k_kinematic_prep<.., HEAT>, k_kinematic_step<.., HEAT>), no run flag and no new call or launch in the step.
 * The heat reads the water and never writes it.  elmkernels_amd/routing.py: heat_tables(), heat_prep(), heat_phi(), heat_settle() and
 * kinematic_call(..., heat=) restate it on the host.
 *
 * Conventions of "kinematic-wave routing": no contraction, left-associated + - *, `/` and sqrt correctly rounded, plain IEEE
 * comparisons, every row fp64 in both builds, a NaN stored as the canonical quiet NaN.  exp is glibc's (elmk_exp on the device).
 * X += y below stands for X = X + (y).
 *
 * Inputs, given once after elmk_routing_kinematic_enable: sublev, 0 .. 14, the soil layer whose temperature the subsurface runoff
 * carries (level 5 + sublev of t_soisno), and shade[ncells] in [0, 1], the share of direct and diffuse shortwave kept off the water
 * (NULL: 0.0 everywhere).
 *
 * Rows: ELMK_ROUTE_TT and ELMK_ROUTE_TR (K, the temperatures of the tributary store and the main channel; the only prognostic rows,
 * TFRZ after the enable) and five diagnostics of the last call in K m3, that is heat divided by RHOCP: ELMK_ROUTE_HEAT (the heat
 * content at the call's end), ELMK_ROUTE_HIN (entered with runoff), ELMK_ROUTE_HSRF (through the water surface), ELMK_ROUTE_HADJ (by
 * the settle rule H5) and ELMK_ROUTE_HOUT (left the cell with the main channel's flow).  elmk_routing_read accepts the seven only while
 * the extension is on.
 *
 * Literals: TFRZ = 273.15, TMAX = 313.15, RHOCP = 4188000.0, EMIS = 0.97, SB = 5.67e-8, ALBW = 0.1, CPAIR = 1004.64, LV = 2.501e6,
 * RAIR = 287.04, CEX = 1.3e-3, DMIN = 1e-3.  fl(t) = t > TFRZ ? t : TFRZ, so a NaN gives TFRZ.
 *
 * H0. (tables) AT = TLEN * TWIDTH;  ACHN = RLEN * RWIDTH;  WMINT = AT * DMIN;  WMINR = ACHN * DMIN;
 *     KSW = (1.0 - ALBW) * (1.0 - SHADE);  EMS0 = (EMIS * SB) / RHOCP.  The host forms KSW and EMS0 once at the enable; the four
 *     products of the scheme's parameters are formed where they are used, from the same operands.
 * H1. (K1 launch, once per call) over the cell's terms in R1's order, the first term assigned and the others added, each term w * x:
 *     TA, PA, QA, LW from x = forc_tbot, forc_pbot, forc_qbot, forc_lwrad;  UA from x = sqrt(forc_u * forc_u + forc_v * forc_v);
 *     SW from x = ((forc_solad[0] + forc_solad[1]) + forc_solai[0]) + forc_solai[1];  TSUR from x = fl(t_grnd);
 *     TSUB from x = fl(t_soisno[5 + sublev]).  Every field is read as stored and widened (the fp32-state build sees its stored values).
 *     A cell with terms: RAD = (KSW * SW + EMIS * LW) / RHOCP;  KE = ((PA / (RAIR * TA)) * CEX) * UA;  EMS = EMS0.
 *     A cell without terms (a pass-through reach): RAD = KE = EMS = 0.0;  TSUR = TSUB = TFRZ;  TA = QA = PA = 0.0.
 *     TEQ = fl(TA).  The five diagnostic rows are zeroed.  The heat-flow row takes hr = er * TR, with er the flow this launch writes.
 * H2. phi(T): d = T - TFRZ;  es = 611.2 * exp((17.67 * d) / (T - 29.65));  qs = (0.622 * es) / (PA - 0.378 * es);  t2 = T * T;
 *     phi = (RAD - EMS * (t2 * t2)) + (KE * (CPAIR * (TA - T) - LV * (qs - QA))) / RHOCP.
 * H3. (tributaries, per sub-step) from the sub-step's start values and K3 / K4's eh, et:
 *     gb = QSUB > 0.0 ? QSUB * TSUB : QSUB * TT;  sx_T = WT > WMINT ? AT * phi(TT) : 0.0;  hi = eh * TSUR + gb;
 *     h = TT * WT + ((hi - et * TT) + sx_T) * dts;  wn = K6's new WT;  (TT, adj_T) = settle(h, wn, WMINT).
 * H4. (main channel) fh = the sum of hr[u] over the upstream slots ascending, from +0.0, as K5 sums er;  ho = hr[c];
 *     sx_R = VOLR > WMINR ? ACHN * phi(TR) : 0.0;  h = TR * VOLR + (((fh - ho) + et * TT) + sx_R) * dts with the TT of the sub-step's
 *     start;  wn = K6's new VOLR;  (TR, adj_R) = settle(h, wn, WMINR).  Every sub-step but the last writes hr = e * TR from the new TR
 *     and the er it forms, into the second of a pair of buffers beside er's.
 * H5. settle(h, wn, wmin): if (wn > wmin) { t = h / wn;  if (!(t >= TFRZ)) t = TFRZ;  if (t > TMAX) t = TMAX; } else t = TEQ;
 *     adj = t * wn - h where the rule has acted - t is TEQ, or one of the two ifs has fired - and +0.0 where t is the quotient itself:
 *     there t * wn is h up to the division's rounding, which is no heat.  A store too thin to hold a temperature takes the air's; a
 *     store driven past the bounds is held at them, and adj is the heat that this adds.
 * H6. (diagnostics) per sub-step, in this order: HIN += hi * dts;  HSRF += (sx_T + sx_R) * dts;  HADJ += adj_T + adj_R;
 *     HOUT += ho * dts.  The last sub-step stores HEAT = TT * WT + TR * VOLR from the new values.
 * H7. (elmk_routing_heat_budget) sums[0 .. 3] = the sums of HEAT, HIN, HSRF and HADJ, sums[4] = the sum of HOUT over the outlets (R6's
 *     outlet rule: down < 0), all through R6's reduction kernels.  Over a call,
 *     sum HEAT at its end - sum HEAT at its start = sums[1] + sums[2] + sums[3] - sums[4], up to rounding
 *     (tests/test_routing_heat_host.py counts the roundings).
 * H8. Every water row keeps the bits of the scheme without the extension.
 * H9. Edge values do what H1 - H6 say literally.  A NaN TT or TR makes h NaN; where wn > wmin, t = NaN fails t >= TFRZ and the store
 *     takes TFRZ, and adj and HADJ are NaN for that call: the temperature recovers, the budget of that call does not.  +inf likewise
 *     (t2 * t2 = +inf, phi = -inf or NaN).  A NaN, zero, negative or subnormal WT or VOLR is not > wmin: no surface exchange, and where
 *     the new storage is not > wmin either the store takes TEQ.  PA == 0.0 gives qs = (0.622 * es) / (-(0.378 * es)), finite and
 *     negative.  A NaN TA makes KE and phi NaN while TEQ = TFRZ.  A cell without terms exchanges nothing through its surface:
 *     phi = +0.0 for every finite T.
 *
 *   elmk_routing_heat_enable  takes the inputs, allocates the rows, H1's rows, KSW and the two hr buffers in one allocation (TT and
 *                           TR TFRZ, the rest zero; counted in elmk_device_bytes) and drops the captured run step.  ELMK_E_INVALID,
 *                           nothing changed: the kinematic scheme not on; already on; the floodplain inundation or the reservoirs on
 *                           ("elmk_routing_inundation_clear first", "elmk_routing_reservoir_clear first"); sublev outside 0 .. 14; a
 *                           shade value not finite or outside [0, 1] (the text names the row and the first offending cell,
 *                           "elmk_routing_heat_enable: SHADE outside [0, 1] at cell 17"); a stream being captured.
 *   elmk_routing_heat_init    TT and TR from host[ncells] (NULL: TFRZ), the diagnostics zero.  Synchronises.
 *   elmk_routing_heat_budget  H7; synchronises.
 *   elmk_routing_heat_clear   back to the scheme without temperatures; frees what enable allocated and drops the captured run step.
 * While the extension is on elmk_routing_kinematic_clear, elmk_routing_inundation_enable and elmk_routing_reservoir_enable are refused
 * with ELMK_E_INVALID ("elmk_routing_heat_clear first"); elmk_routing_clear frees everything.  elmk_routing and elmk_run with
 * ELMK_RUN_ROUTING run the HEAT form while it is on.
 * Tapes: elmk_cell_history_add_row(ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_TT .. ELMK_ROUTE_HOUT) works while the extension is on, and while
 * such an entry exists elmk_routing_heat_clear is refused ("elmk_history_clear first").
 * Restart: under ELMK_OPT_RESTART_CELLS a context with the heat on saves an image of version 8 (ELMK_RESTART_VERSION_HEAT): version 6
 * plus the cell sections ELMK_ROUTE_TT and ELMK_ROUTE_TR after WT; it loads only into a context with the same stages on, and the load
 * leaves the diagnostics zero; every other context saves byte for byte what it saved before.  With the option off a driver saves TT
 * and TR with elmk_routing_read and hands them to elmk_routing_heat_init after elmk_routing_heat_enable.  A context that never calls
 * these entries runs the kernels, launch sequences and graphs it ran before and allocates nothing more.
 * Out of scope, each a later change: heat on the floodplain and in a stratified reservoir (hence the interlock), river ice, a heat
 * store on the hillslope, and the linear scheme. */
enum { ELMK_ROUTE_TT = 13, ELMK_ROUTE_TR = 14, ELMK_ROUTE_HEAT = 15, ELMK_ROUTE_HIN = 16,
       ELMK_ROUTE_HSRF = 17, ELMK_ROUTE_HADJ = 18, ELMK_ROUTE_HOUT = 19 };
int elmk_routing_heat_enable(elmk_ctx *ctx, int sublev /*0 .. 14*/, const double *shade /*[ncells] or NULL: 0.0*/);
int elmk_routing_heat_init(elmk_ctx *ctx, const double *tt /*[ncells] or NULL: TFRZ*/, const double *tr /*[ncells] or NULL: TFRZ*/);
int elmk_routing_heat_budget(elmk_ctx *ctx, double *sums /*[5]: H7, through R6's reduction kernels*/);
int elmk_routing_heat_clear(elmk_ctx *ctx);

/* ---- floodplain infiltration ------------------------------------------------------------------------
 * The river-to-land coupling of the floodplain inundation (ELM's use_lnd_rof_two_way: the h2orof / frac_h2orof inputs of
 * SoilHydrologyMod::Infiltration, with qflx_h2orof_drain going back to MOSART): the water standing on a flooded cell infiltrates the soil
 * columns under it, and the routing takes what infiltrated out of the floodplain store.  An opt-in extension of the soil hydrology, the
 * water balance and the kinematic-wave routing: template forms of their kernels, no run flag, no new launch.  The conventions are those of
 * "soil hydrology" and "kinematic-wave routing": no contraction, left-associated + - *, `/` correctly rounded, plain IEEE comparisons,
 * every row fp64 in both builds, a NaN stored into a row is the canonical quiet NaN.
 * elmk_floodplain_infiltration_enable needs, and refuses with ELMK_E_INVALID and nothing changed otherwise (the text says which): the
 * soil hydrology on, the water balance on, the kinematic-wave routing on, the floodplain inundation on, every column in at most one
 * output cell (the refusal names the first shared column), no stream being captured, not already on.  The stream temperature is excluded
 * through the inundation's own interlock; the reservoirs may be on.
 *   F0 (host, once at enable) cellof[ncols], int32: the cell whose CSR span names column c, or -1 for a column in no cell; kept on the
 *      device, owned by the extension and counted in elmk_device_bytes.
 *   F1 (soil hydrology, section C, after qinmax is formed)
 *        g = cellof[c];  if (g >= 0) { wf = WF[g]; ff = FLOOD_FRAC[g]; ar = area[g]; }
 *        if (g >= 0 && wf > 0.0 && ff > 0.0 && ar > 0.0) {
 *          hr = (wf / ar) * 1000.0                  mm over the cell's area
 *          a = ff * qinmax;  b = hr / dt;  d = (a < b) ? a : b
 *        } else { hr = 0.0; d = 0.0 }
 *      WF and FLOOD_FRAC are read as the last routing call or elmk_routing_inundation_init left them: the previous step's end, the
 *      convention of the supply limit's VOLR.  The guard keeps a NaN, zero or negative WF from producing a negative drain.
 *   F2 (the last statement of section C, after infl = infl + drain_sfc)  infl = infl + d.  Sections D to H are unchanged; QFLX_INFL
 *      carries the term.
 *   F3 three fp64 column rows of the extension, each [elmk_level_stride], overwritten every step: ELMK_FPI_H2OROF = hr (mm),
 *      ELMK_FPI_FRAC = ff where the guard passed, else 0.0, ELMK_FPI_QFLX_DRAIN = d (mm/s; ELM's qflx_h2orof_drain).
 *   F4 (water balance, W4) (forc_rain + forc_snow) + QFLX_H2OROF_DRAIN takes the place of forc_rain + forc_snow; with the irrigation on
 *      ((forc_rain + forc_snow) + QFLX_IRRIG) + QFLX_H2OROF_DRAIN.  W3 and QRUNOFF are unchanged.
 *   F5 (routing, the K1 launch, once per call) t = the aggregate of w[p] * QFLX_DRAIN[col[p]] over the cell's terms in R1's order (the
 *      first term assigned, the others added; a cell without terms takes 0.0);  QLAND = (t * 0.001) * area;  WF = WF - QLAND * dt.
 *      ELMK_ROUTE_QLAND is a diagnostic cell row, m3/s.  WF may go slightly negative, as VOLR may with the withdrawal on; F1's guard and
 *      I1 to I4 then do what they say literally.  I6 stands: this launch does no exchange.
 *   F6 elmk_floodplain_infiltration_budget: sums[0] = the sum of QLAND through R6's reduction kernels.  The change of sum WH + sum WT +
 *      sum VOLR + sum WF (+ sum RES) over a call becomes dt (sum QIN - sum outlet QOUT - sum QLAND) (- sum RES_TAKE).
 *   F7 The two sides agree when the hydrology and the routing take the same dt and there is one routing call per hydrology call.
 *      elmk_run guarantees both; stepwise it is the caller's contract, as it is for QRUNOFF and QFLX_IRRIG.
 *   F8 Edge values do what F1 and F5 say literally.  NaN qinmax: a < b is false, so d = b.  WF = +inf: hr = +inf, d = a.  NaN area: the
 *      guard fails.  A column in no cell: d = 0.0, and every other output keeps the bits of the plain stage.  A context in which no cell
 *      is flooded keeps the bits of the stage without the extension on every existing row, column and cell.
 * elmk_floodplain_infiltration_read copies columns [col0, col0 + n) of one of the three column rows; elmk_routing_read takes
 * ELMK_ROUTE_QLAND only while the extension is on.  The three column rows and QLAND are diagnostics that the next step rewrites: there is
 * no new prognostic row.  Restart: WF is in version 6 and later; F1 also reads FLOOD_FRAC as the last routing call left it, a
 * diagnostic that a load leaves zero, so under ELMK_OPT_RESTART_CELLS a context with the extension on saves one more cell section,
 * ELMK_ROUTE_FLOOD_FRAC, behind the others (the version stays what the other stages make it); such an image loads only into a context
 * with the extension on, and 3 + 3 steps through it give the bits of 6.  Every other context saves byte for byte what it saved before.
 * With the option off elmk_routing_inundation_init leaves FLOOD_FRAC zero, so the first step after such a restart drains nothing.
 * While the extension is on elmk_routing_inundation_clear, elmk_soil_hydrology_clear, elmk_water_balance_clear, elmk_set_output_grid and
 * elmk_clear_output_grid are refused with ELMK_E_INVALID ("elmk_floodplain_infiltration_clear first"); elmk_routing_clear frees it with
 * the rest.  Enable and clear drop the captured run step.
 * Tapes: ELMK_ROWS_FLOODPLAIN (which = ELMK_FPI_*) for elmk_column_history_add_row / elmk_gridded_history_add_row, and
 * elmk_cell_history_add_row(ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_QLAND), both while the extension is on; while such an entry exists
 * elmk_floodplain_infiltration_clear is refused ("elmk_history_clear first").
 * A context that never enables it runs the kernels, launch sequences and graphs it ran before, allocates nothing more and saves the image
 * it saved before.  Out of scope: evaporation from floodplain water, which needs an energy balance of its own. */
enum { ELMK_FPI_H2OROF = 0, ELMK_FPI_FRAC = 1, ELMK_FPI_QFLX_DRAIN = 2, ELMK_FPI_NROWS = 3 };
enum { ELMK_ROUTE_QLAND = 20 };
int elmk_floodplain_infiltration_enable(elmk_ctx *ctx);
int elmk_floodplain_infiltration_read(elmk_ctx *ctx, int which /*ELMK_FPI_**/, double *host, int64_t col0, int64_t n);
int elmk_floodplain_infiltration_budget(elmk_ctx *ctx, double *sums /*[1]: the sum of QLAND, through R6's reduction kernels*/);
int elmk_floodplain_infiltration_clear(elmk_ctx *ctx);

/* ---- command areas ----------------------------------------------------------------------------------
 * An opt-in part of the river stage on top of "reservoirs", after MOSART-WM's dependency database (Voisin et al., Hydrol. Earth Syst.
 * Sci. 17, 2013): a dam supplies the cells that depend on it, not only the cell it stands in.  What the own dam (D2) has not covered
 * of a cell's withdrawal is asked of up to ELMK_CMD_NDEP dams, each dam allots what it can among its dependents in proportion, and
 * the cells' QIN is credited with what they received.  It needs the kinematic scheme, the reservoirs and the routing's withdrawal.  No
 * run flag and no new call in the step: while it is on, elmk_routing and the ELMK_RUN_ROUTING stage enqueue two more launches between
 * the K1 launch and the first sub-step (k_routing.hip: k_command_allot, k_command_take), the K1 launch takes its CMD form, and with the
 * river supply limit also on k_irrigation_supply takes its CMD form.  elmkernels_amd/routing.py: check_command(), command_tables(),
 * command_allot(), command_take() and kinematic_call(..., dam={..., "command": cmd}) restate it on the host.
 *
 * Conventions of "reservoirs": no contraction, left-associated + - *, `/` correctly rounded, plain IEEE comparisons, every row fp64 in
 * both builds, a NaN stored as the canonical quiet NaN.
 *
 * Inputs, given once: three ELL rows [ELMK_CMD_NDEP][ncells].  dam: int32, the cell index of a supplying dam, -1 for an empty slot; the
 * slots are filled from slot 0 without gaps.  share: the fraction of the cell's remaining withdrawal that it asks of that dam.  claim:
 * the cell's fixed right to that dam's usable storage at the daily check of the river supply limit (C6).  The host checks them, per
 * cell in index order and per slot in slot order: the index inside [-1, ncells); no filled slot behind an empty one; the named cell has
 * CAP > 0.0; it is not the cell itself (D2 serves the own cell); it is not named by an earlier slot; share finite and in (0, 1]; claim
 * finite and in [0, 1]; then the cell's shares, added in slot order, <= 1.0.  Then the host builds the inverse map: the dam list is
 * every cell with CAP > 0.0 in ascending order (a dam without dependents has an empty span), and a CSR over that list holds the terms
 * (cell, slot) sorted by cell and then slot; every dam's claims, added in term order, must be <= 1.0.  Linear time, no recursion.  Dam
 * indices are a context's own cells: with several ranks a context allots among the cells it holds.
 *
 * Rows, all fp64 diagnostics that every call overwrites, zero after the enable except RATIO, which is 1.0: ELMK_ROUTE_CMD_WANT (m3, what
 * a dependent cell asks for in total), ELMK_ROUTE_CMD_TAKE (m3, what it received), and at a dam's cell ELMK_ROUTE_CMD_GIVE (m3, what
 * the dam gave) and ELMK_ROUTE_CMD_RATIO (the dam's ratio).  elmk_routing_read accepts the four only while the part is on.  There is no
 * prognostic row: no image version changes, and with ELMK_OPT_RESTART_CELLS a context with the part on saves the version-7 image byte
 * for byte (a load leaves WANT, TAKE and GIVE zero and RATIO 1.0).
 *
 * C0. A cell with no filled slot, and a dam with no terms, keep every bit of the form without the part; such a cell's WANT and TAKE and
 *     such a dam's GIVE and RATIO are not written.
 * C1. (K1 launch, k_kinematic_prep_cmd, the CMD form of the K1 launch, which exists only with the withdrawal and the reservoirs) a cell with a filled
 *     slot forms, after R1 and D2, with iv = (i * 0.001) * area: for a dam cell rest = iv - t / dt (D2's t), for any other cell
 *     rest = iv;  WANT = rest > 0.0 ? rest * dt : 0.0.  QIN, QSUB, D1 - D3 and the first er are what they are without the part.
 * C2. (k_command_allot, one sum per dam with terms) RES here is what the K1 launch left: after D1, D2 and the first D3.
 *     W = the sum over the dam's terms in CSR order of x = share * WANT[cell], the first term assigned and the rest added;
 *     a = RES - SMIN;  avail = a > 0.0 ? a : 0.0;  ratio = W > avail ? avail / W : 1.0;  G = W * ratio;  RES = RES - G;  GIVE = G;
 *     RATIO = ratio.
 * C3. (k_command_take, one thread per cell) a cell with a filled slot forms got = the sum in slot order of (share * WANT) * RATIO[dam] -
 *     the product x of C2, one rounding, then the ratio; the first slot assigned and the rest added;  TAKE = got;
 *     QIN = QIN + got / dt;  QSUB = QIN - QSUR.
 * C4. The sub-steps run unchanged; D3 of the later sub-steps sees the reduced RES.
 * C5. (elmk_routing_command_budget) sums[0] = the sum of CMD_GIVE, sums[1] = the sum of CMD_TAKE, through R6's reduction kernels.  The
 *     change of sum WH + sum WT + sum VOLR (+ sum WF) + sum RES over a call = dt (sum QIN - sum outlet QOUT) - sum RES_TAKE - sum
 *     CMD_GIVE, and sum CMD_GIVE and sum CMD_TAKE agree but for the roundings: every term x * ratio is rounded once where it is taken,
 *     G once per dam, and each sum once per addition.
 * C6. (river supply limit, k_irrigation_supply<DAM, CMD>; elmkernels_amd/irrigation.py: supply_limit(command=)) S3 for a cell with
 *     filled slots: after D7's own-dam term and before `- Vc`, for each slot in order r = RES[dam] - SMIN[dam], taken as 0.0 unless
 *     > 0.0, and a = a + claim * r.  Every other cell keeps D7 / S3, and so does every cell with the part off.
 * C7. Guaranteed: the claims of a dam sum to at most 1, so one check never promises more than the dam's usable storage.  Not
 *     guaranteed: storage that is drawn down between a grant and its withdrawal - by D3's releases, by D2, by other cells' takes.  C2's
 *     ratio catches that: what the dam cannot give leaves the channel, as in R1.
 * C8. Edge values do what C1 - C3 say literally.  A NaN RES gives a = NaN, avail = 0.0: ratio = 0.0 for W > 0 (G = 0.0, RES stays NaN),
 *     1.0 for W = 0.  RES = +inf gives everything asked (ratio 1.0) and stays +inf; RES = -inf, a negative RES and any RES <= SMIN
 *     have avail = 0.0 and give nothing (ratio 0.0 for W > 0: G = W * 0.0 = 0.0).  WANT = +inf in a term makes W = +inf: with a finite
 *     avail ratio = 0.0 and G = inf * 0.0 = NaN, so RES, GIVE and every dependent's TAKE and QIN are NaN; with avail = +inf too, W > avail
 *     fails, ratio = 1.0 and G = +inf, RES = NaN.  W = 0 with terms fails W > avail: ratio = 1.0, G = 0.0, and RES - 0.0 keeps RES
 *     (but -0.0 stays -0.0).  A NaN i makes rest NaN, which fails rest > 0.0: WANT = 0.0, nothing is asked, while QIN is NaN as it
 *     is without the part.
 *
 *   elmk_routing_command_enable  checks the rows, builds the inverse map, allocates and uploads everything (one owner, counted in
 *                           elmk_device_bytes) and drops the captured run step.  ELMK_E_INVALID, nothing changed: the kinematic
 *                           scheme, the reservoirs or the routing's withdrawal off; already on; a null argument; a bad value (the
 *                           text names the row and the first offending cell - for a dam's claims the dam's cell - as in
 *                           "elmk_routing_command_enable: SHARE outside (0, 1] at cell 17"); a stream being captured.
 *   elmk_routing_command_budget  C5; synchronises.
 *   elmk_routing_command_clear   back to dams that serve their own cell; frees what enable allocated and drops the captured run
 *                           step.  From then on every row takes the bits of a context that never had the part, given the same RES.
 * While the part is on elmk_routing_reservoir_clear and elmk_routing_set_withdrawal(ctx, 0) are refused with ELMK_E_INVALID
 * ("elmk_routing_command_clear first"); elmk_routing_clear frees everything.  The river supply limit may be enabled and cleared in
 * either order relative to the part.
 * Tapes: elmk_cell_history_add_row(ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_CMD_*) works while the part is on, and while such an entry exists
 * elmk_routing_command_clear is refused ("elmk_history_clear first").
 * A context that never enables it runs the kernels, launch sequences and graphs it ran before, allocates nothing more and saves the image
 * it saved before. */
enum { ELMK_CMD_NDEP = 4 };
enum { ELMK_ROUTE_CMD_WANT = 21, ELMK_ROUTE_CMD_TAKE = 22, ELMK_ROUTE_CMD_GIVE = 23, ELMK_ROUTE_CMD_RATIO = 24 };
int elmk_routing_command_enable(elmk_ctx *ctx, const int32_t *dam /*[4][ncells]*/, const double *share /*[4][ncells]*/,
                                const double *claim /*[4][ncells]*/);
int elmk_routing_command_budget(elmk_ctx *ctx, double *sums /*[2]: the sums of CMD_GIVE and CMD_TAKE, through R6's reduction kernels*/);
int elmk_routing_command_clear(elmk_ctx *ctx);

/* ---- feature rows on history tapes --------------------------------------------------------------
 * elmk_history_add and elmk_gridded_history_add take state fields; what the features above produce lives in fp64 rows beside the state.
 * These two entries register one such row, over the columns (elmk_column_history_add_row; the six elmk_history_* entries of "history"
 * stay the set they are) or over the output grid's cells: as elmk_history_add / elmk_gridded_history_add (the same entry ids, table, limits, ops,
 * refusals and fold semantics, still one elmk_history_accumulate launch), one level, the sample the row's fp64 value in both builds.
 * family: ELMK_ROWS_ALT (which = ELMK_ALT_*), ELMK_ROWS_HYDROLOGY (ELMK_HYD_*), ELMK_ROWS_FROST (ELMK_HYDF_*), ELMK_ROWS_WATER_BALANCE
 * (ELMK_WB_*), ELMK_ROWS_IRRIGATION (ELMK_IRR_*).  Refused as well: an unknown family, a family that is not enabled, `which` out of range.
 * While a row entry exists the *_clear of its family is refused with ELMK_E_INVALID ("elmk_history_clear first") and nothing changes:
 * elmk_soil_hydrology_clear for the hydrology, the frost-table extension and the water balance, elmk_soil_hydrology_frost_clear and
 * a second elmk_soil_hydrology_frost_enable for the extension.  This mirrors elmk_clear_output_grid under gridded entries.
 * Restart: a row entry is saved and loaded like any history entry; its elmk_restart_entry.field holds
 * ELMK_RESTART_ROW_FIELD(family, which), a value no field id reaches, so a loader from before row entries refuses the image as a
 * history table other than its own.  Images of contexts without row entries are what they were. */
enum { ELMK_ROWS_ALT = 0, ELMK_ROWS_HYDROLOGY = 1, ELMK_ROWS_FROST = 2, ELMK_ROWS_WATER_BALANCE = 3, ELMK_ROWS_IRRIGATION = 4, ELMK_ROWS_NFAMILY = 5 };
/* the floodplain infiltration's three column rows (which = ELMK_FPI_*): the family's number lies past the cell-row families', which the
 * restart image numbers from ELMK_ROWS_NFAMILY on, so that every image keeps the numbers it had */
enum { ELMK_ROWS_FLOODPLAIN = 7 };
/* the hillslope lateral flow's six column rows (which = ELMK_HS_*): the next number no family and no image uses */
enum { ELMK_ROWS_HILLSLOPE = 8 };
#define ELMK_RESTART_ROW_BASE 0x40000000
#define ELMK_RESTART_ROW_FIELD(family, which) (ELMK_RESTART_ROW_BASE + ((family) << 16) + (which))
int elmk_column_history_add_row(elmk_ctx *ctx, int tape, int family, int which, int op);
int elmk_gridded_history_add_row(elmk_ctx *ctx, int tape, int family, int which, int op);

/* ---- cell rows on history tapes -----------------------------------------------------------------
 * What the river stages produce lives in fp64 rows over the output grid's CELLS, which neither entry above reaches.  This one registers
 * such a row: as elmk_history_add (the same entry table, ids, ops, tapes, limits and refusals, the fold semantics of "history" word for
 * word - SUM / AVG from -0.0, MAX / MIN from -/+inf with a sticking NaN, INST the last sample, AVG divided once when read - and still
 * ONE elmk_history_accumulate launch, in elmk_run's ELMK_RUN_HISTORY stage too, where it follows the routing stage: the sample of step
 * k is the routing's result of step k), one level, the sample the row's fp64 value in both builds.
 * family: ELMK_CELL_ROWS_ROUTING (which = ELMK_ROUTE_*: exactly the rows elmk_routing_read accepts at the moment of the call - WH, WT,
 * QSUR only while the kinematic-wave scheme is on, WF, FLOOD_DEPTH, FLOOD_FRAC only while the floodplain inundation is on) or
 * ELMK_CELL_ROWS_SUPPLY (which = ELMK_IRRSUP_*, while the river supply limit is on).  Refused as well: an unknown family, a family that
 * is not enabled, `which` out of range.
 * Unlike a gridded entry it has no map and no fill: EVERY cell is a sample, a cell without columns in the output grid's map included (a
 * pass-through reach still has storage and flow).  The accumulators are ncells rounded up to 64 doubles, counted in elmk_device_bytes.
 * elmk_history_read on such an entry indexes cells (col0, n within ncells) and ignores `layout`; elmk_history_reset, _count and _clear
 * treat it as every other entry.
 * While such an entry exists, the call that would free its source row or change ncells is refused with ELMK_E_INVALID
 * ("elmk_history_clear first") and nothing changes: elmk_routing_clear; elmk_routing_kinematic_clear under entries on WH, WT, QSUR
 * (and, through the inundation's own interlock, on the flood rows); elmk_routing_inundation_clear; elmk_irrigation_supply_clear;
 * elmk_set_output_grid and elmk_clear_output_grid.  The _init and _reset_mean calls stay allowed: they write values, not pointers.
 * Restart: saved and loaded like any history entry; elmk_restart_entry.field = ELMK_RESTART_ROW_FIELD(ELMK_ROWS_NFAMILY + family,
 * which), gridded = 2, ncells the routing's, the accumulators an ELMK_RESTART_GRIDDED section of extent ncells.  Images of contexts
 * without such entries are what they were.  The source rows themselves (VOLR, WH, ...) are in the image only under
 * ELMK_OPT_RESTART_CELLS (version 6, "restart"); else the driver carries them through the _read / _init pairs of the river stages.
 * Later changes: a per-step series of chosen cells (a gauge hydrograph), cell data across a change of decomposition. */
enum { ELMK_CELL_ROWS_ROUTING = 0, ELMK_CELL_ROWS_SUPPLY = 1, ELMK_CELL_ROWS_NFAMILY = 2 };
int elmk_cell_history_add_row(elmk_ctx *ctx, int tape, int family, int which, int op);

/* ---- point series -----------------------------------------------------------------------------------
 * Per-step records of chosen columns and river cells: the series at a flux-tower site (latent heat, t_grnd, ZWT every half hour), the
 * hydrograph at a gauge cell (QOUT, VOLR, TR, RES every step), a site's gridcell mean - what the tapes of "history" average away and
 * what "cell rows on history tapes" named as its later change.  An opt-in part: a driver names a few points and a few sources once;
 * every record is ONE launch that gathers the current value of every (source, point) pair into a device-resident ring
 * [max_records][values] with a time stamp per record, and the records are read back in bulk whenever the driver likes.  A context that
 * never calls these entry points enqueues the launches it did and saves the images it did.  elmkernels_amd/points.py restates P1 - P3
 * in numpy (record(), ring()).
 *   P0  sources and entries.  An entry is one source; its points are the list of its kind: the columns list (ELMK_POINTS_COLUMNS) for
 *       elmk_points_add_field and _add_row, the cells list (ELMK_POINTS_CELLS, the output grid's cells, which are the routing's) for
 *       _add_cell_row, _add_gridded_field and _add_gridded_row.  The sources accepted are exactly those the history entry points accept
 *       at the moment of the call - elmk_history_add for one level, elmk_column_history_add_row, elmk_cell_history_add_row,
 *       elmk_gridded_history_add / _add_row for one level - with the same refusals: an unknown field, a level out of range, a family
 *       that is not enabled, `which` out of range, no output grid.  Entries and lists may change only while total == 0: before the first
 *       record or after elmk_points_reset.  A list is copied, in any order, duplicates allowed.
 *   P1  sample.  The stored value widened to fp64 exactly as "history" widens it: F64 as stored (fp32 widened in libelmk_f32.so), I32, U8
 *       and U32 exactly, rows as their fp64 value.  NaN payloads, infinities and -0.0 arrive bit for bit.
 *   P2  gridded sample.  elmk_download_gridded's value for that one cell: fill where ptr[i] == ptr[i+1], else v = w[p0] * x[col[p0]], then
 *       v = v + w[p] * x[col[p]] in term order, no contraction, one lane taking the sum.
 *   P3  record.  Record number r (0-based since the last reset) lands in slot r % max_records.  A slot holds the stamp and, per entry,
 *       npoints doubles in list order (entries padded so that one wave never straddles two).  held = min(total, max_records);
 *       elmk_points_read and _stamps index the held records oldest first, rec0 + nrec <= held.  A record writes nothing but its slot.
 *   P4  stepwise.  elmk_points_record(ctx, stamp) is ONE launch on the context's stream: no host memory, no synchronisation.  Refused,
 *       nothing enqueued: without a reservation, without entries, with an entry whose list is empty, on a stream being captured.
 *   P5  in a run.  While elmk_points_set_run(ctx, 1) is in force every step of elmk_run records once, after the history stage and before
 *       the cursor moves: the sample of step s is what the step left, the routing's result included; the stamp is the step's decday.  No
 *       run flag and no member of elmk_run_step: one more launch is enqueued behind the history's, and a captured step is keyed by it.
 *       Record numbers continue across runs and across stepwise records in between; run k+1 enqueued while run k executes gives the same
 *       series.  An armed elmk_run is refused, nothing enqueued, where P4 refuses a record.
 *   P6  counting.  The number of records is known on the host when a record is enqueued: no device counter.  In a replayed graph the
 *       slot is not baked into the captured arguments: the kernel derives it from the run's step cursor and a base word that elmk_run
 *       writes on the stream before the run's first step.  elmk_points_count does not synchronise; _read and _stamps do.
 *   P7  interlocks.  While an entry exists, a call that would free or resize what it reads is refused with ELMK_E_INVALID
 *       ("elmk_points_clear first") and changes nothing: the clears that row, cell-row and gridded history entries guard, and
 *       elmk_set_output_grid / elmk_clear_output_grid under gridded or cell-row entries or a cells list.  elmk_points_set checks every
 *       index against ncols, or against the output grid's ncells; the refusal names the first offending position and value.
 *   P8  memory.  Everything is counted in elmk_device_bytes and returned by elmk_points_clear.  The restart image does not change in any
 *       version: the series is output, not state; a driver reads it before it saves.
 *   P9  untouched contexts.  A context without a reservation runs the kernels, launch sequences and graphs it ran before;
 *       elmk_points_set_run(ctx, 0), _reset and _clear give back the launch sequence of a context that never had the part.
 *
 *   elmk_points_set         the list of `kind` (n <= ELMK_POINTS_MAX_POINTS; n = 0 empties it).  The cells list needs the output grid.
 *   elmk_points_add_*       one entry; returns its id (>= 0, in order of registration), at most ELMK_POINTS_MAX_ENTRIES.
 *   elmk_points_reserve     the ring: max_records in 1 .. 2^24 records of the present entries (resized with them while total == 0).
 *   elmk_points_record      P4.
 *   elmk_points_set_run     P5; switching it on needs a reservation.
 *   elmk_points_count       total (records since the last reset) and held; either pointer may be NULL.
 *   elmk_points_read        host[nrec][npoints] of one entry, held records rec0 .. rec0 + nrec - 1; synchronises.
 *   elmk_points_stamps      host[nrec], the same records' stamps; synchronises.
 *   elmk_points_reset       total back to 0 (the next record lands in slot 0) and the run's recording off; entries, lists and the
 *                           reservation stay.  Synchronises.
 *   elmk_points_clear       frees everything: entries, lists, reservation, the armed state.
 * All but elmk_points_record and _count are refused on a stream being captured. */
enum { ELMK_POINTS_COLUMNS = 0, ELMK_POINTS_CELLS = 1, ELMK_POINTS_NKIND = 2 };
#define ELMK_POINTS_MAX_ENTRIES 64
#define ELMK_POINTS_MAX_POINTS 4096 /* per kind */
int elmk_points_set(elmk_ctx *ctx, int kind, int64_t n, const int64_t *idx /*[n]*/);
int elmk_points_add_field(elmk_ctx *ctx, int field, int level);
int elmk_points_add_row(elmk_ctx *ctx, int family, int which);
int elmk_points_add_cell_row(elmk_ctx *ctx, int family, int which);
int elmk_points_add_gridded_field(elmk_ctx *ctx, int field, int level);
int elmk_points_add_gridded_row(elmk_ctx *ctx, int family, int which);
int elmk_points_reserve(elmk_ctx *ctx, int max_records);
int elmk_points_record(elmk_ctx *ctx, double stamp);
int elmk_points_set_run(elmk_ctx *ctx, int on);
int elmk_points_count(elmk_ctx *ctx, int64_t *total, int64_t *held);
int elmk_points_read(elmk_ctx *ctx, int entry, double *host /*[nrec][npoints]*/, int64_t rec0, int64_t nrec);
int elmk_points_stamps(elmk_ctx *ctx, double *host /*[nrec]*/, int64_t rec0, int64_t nrec);
int elmk_points_reset(elmk_ctx *ctx);
int elmk_points_clear(elmk_ctx *ctx);

/* ---- restart ---------------------------------------------------------------------------------
 * Exact restarts (E3SM's ERS test: 2N steps give the bits of N steps, a restart, N more steps).  A context saves its column state
 * and history into a self-describing byte buffer, the image, and another context - in another process, or with another column
 * decomposition through elmkernels_amd/restart.py - loads it.  Continuing from the load gives the bits of the run that never stopped.
 *
 * Which fields an image holds comes from one table, include/elmk_restart.def, read through elmk_field_class.  Classes are relative to
 * one model step (the per-step sequence of elmk_run): PROGNOSTIC - some element may be read before the step writes it, or survive the
 * step unwritten (err_flags included: its bits are sticky); SURFACE - read and never written by the step (soil hydraulics, geometry,
 * what elmk_initialize_state derives, land and plant-type indices); FORCING - the series fields atm_tbot .. atm_wind and mlai .. mhbot,
 * which the driver supplies every step; DIAGNOSTIC - every element is overwritten by the step before any read.  The image holds the
 * PROGNOSTIC and SURFACE fields.
 *
 * Image format, version 1.  Little-endian; all offsets from the start of the image.
 *   elmk_restart_header at 0, then nentries elmk_restart_entry (the history entries in registration order), then nsections
 *   elmk_restart_section; zero padding up to header_bytes (a multiple of 256).  Then the sections, in table order, each at a
 *   256-byte aligned offset, dense [nlev][extent] in its element type, zero padding up to the next multiple of 256:
 *     ELMK_RESTART_FIELD    id = field id, extent = ncols, the field's ABI element type: F64 fields as doubles in both builds
 *                           (libelmk_f32.so widens its fp32 values exactly as elmk_download does); one per PROGNOSTIC or
 *                           SURFACE field, in field id order
 *     ELMK_RESTART_HISTORY  id = entry index, extent = ncols, F64: the raw accumulators (not acc / count)
 *     ELMK_RESTART_GRIDDED  id = entry index, extent = ncells of the output grid, F64: the cell accumulators
 *     ELMK_RESTART_ACCUM    (version 2) id = accumulator entry index, extent = ncols, F64: the value rows of elmk_accum_add
 *   Checksum of a section: the sum modulo 2^64 of term = fmix64(bits ^ fmix64(g * 64 + lev + 1)) over its elements, fmix64 the
 *   murmur3 finalizer, bits the element zero-extended to 64 bits, g the global column (gcol0 + column; the cell for GRIDDED), lev
 *   its level.  A sum, so it is the same in any reduction order, and images of adjacent column ranges merge by adding checksums.
 *   Checksum of the header: the same sum over the 8-byte words w_i of [0, header_bytes), header_checksum read as 0, with g = i,
 *   lev = 0.  schema_hash: FNV-1a 64 over, for every field in id order, its name, a 0 byte, its dtype byte and its nlev byte.
 *
 * Image format, version 2: what a context WITH accumulator entries (elmk_accum_add) saves; one without saves version 1, byte for
 * byte as before.  As version 1, except that header.version = 2, the 8-byte word after the header holds the number of accumulator
 * entries (uint32, then a zero uint32), the history entries follow it, then one elmk_restart_accum per accumulator entry in
 * registration order (source, kind, destination, period and the step count n), then the section table; the ELMK_RESTART_ACCUM
 * sections come last, checksummed as the other column sections.  The header checksum covers all of it.
 *
 * Image format, version 3: what a context with the active layer thickness enabled (elmk_active_layer_enable) saves.  As version 2,
 * with the accumulator-count word always present (0 without entries), and after the ELMK_RESTART_ACCUM sections three sections of kind
 * ELMK_RESTART_ALT, id = ELMK_ALT_ALT, ELMK_ALT_ALTMAX, ELMK_ALT_ALTMAX_LASTYEAR, nlev = 1, F64, extent = ncols: the three rows,
 * checksummed as the other column sections.  A version-3 image loads only into a context with the feature enabled, a version-1 or
 * version-2 image only into one without it.
 *
 * Image format, version 4: what a context with the soil hydrology enabled (elmk_soil_hydrology_enable) saves.  As version 3, with the
 * ELMK_RESTART_ALT sections present exactly when the active layer thickness is enabled too (the section table says which optional kinds
 * an image holds), and last two sections of kind ELMK_RESTART_HYDROLOGY, id = ELMK_HYD_ZWT, ELMK_HYD_WA, nlev = 1, F64, extent = ncols.
 * A version-4 image loads only into a context with the same features enabled; the parameter rows are not part of it.
 *
 * Image format, version 5: what a context with the irrigation enabled (elmk_irrigation_enable) saves.  As version 4, with each optional
 * kind present exactly when its feature is enabled, and last two sections of kind ELMK_RESTART_IRRIGATION, id = ELMK_IRR_RATE,
 * ELMK_IRR_NLEFT, nlev = 1, F64, extent = ncols.  A version-5 image loads only into a context with the same features enabled; sched is
 * not part of it.
 *
 * Image format, version 6: what a context with the runoff routing enabled (elmk_routing_enable) saves WHILE ELMK_OPT_RESTART_CELLS is on
 * (elmk_set_option); with the option off such a context saves what it saved before, and the driver carries the river stages' rows by
 * hand through their _read / _init pairs.  As version 5, with each optional kind present exactly when its feature is enabled; a second
 * 8-byte word follows the accumulator-count word and holds the routing's call count (int64: elmk_routing_count); and last come the CELL
 * sections of the routing state, nlev = 1, F64, extent = the routing's ncells, checksummed as ELMK_RESTART_GRIDDED sections are (g = the
 * cell, not gcol0 + it): kind ELMK_RESTART_ROUTING with id = ELMK_ROUTE_VOLR and ELMK_ROUTE_QOUT_SUM always, ELMK_ROUTE_WH and
 * ELMK_ROUTE_WT exactly while the kinematic-wave scheme is on and ELMK_ROUTE_WF exactly while the floodplain inundation is on, in that
 * order; then one section of a second kind, ELMK_RESTART_IRRSUP, id = ELMK_IRRSUP_UNMET_SUM, exactly while the river supply limit is on.
 * A version-6 image loads only into a context with the option on, the routing enabled with the same ncells and the same scheme,
 * extension and limit on; a context with the option on and the routing enabled refuses every older image.  After the load the
 * diagnostic rows (QIN, QOUT, QSUR, FLOOD_DEPTH, FLOOD_FRAC, DEMAND, COMMITTED, RATIO) are zero, as after the _init calls, and the call
 * count is the image's: the restart order is "enable the river stages, add the history entries, elmk_restart_load", with no _init call.
 * The network, the parameters and the tables are not part of the image.  elmkernels_amd/restart.py refuses to merge or slice a
 * version-6 image: cell data does not follow a column decomposition (a later change).
 *
 * elmk_restart_size: bytes of this context's image.  elmk_restart_save: the image of the context's columns, which are global
 * columns [gcol0, gcol0 + ncols) of the run.  elmk_restart_load: verifies the whole image on the device (every checksum, snl in
 * 0..nlevsno, as elmk_upload) before it writes anything, then writes the fields, the accumulators, the tape counts and the
 * accumulated fields' value rows and step counts; a tape with count > 0 counts as accumulated (elmk_history_add refuses it until
 * its reset).  Both synchronise with the context's stream and any elmk_run in flight; staging memory is allocated for the call and
 * freed before it returns.  ELMK_E_INVALID, with state, history and counts untouched and the context usable, for: a stream being
 * captured, a too small or truncated buffer, a bad magic
 * or version, another schema, another ncols or gcol0, a history entry table other than the context's (same entries, same order,
 * gridded entries with the same ncells), an accumulator table other than the context's (same source, kind, period and destination,
 * same order; the counts are loaded, not compared), a version-3 image without the active layer thickness enabled or an older one with
 * it, any checksum mismatch, snl out of range.
 *
 * The image holds column data and history only.  Parameters, SNICAR and snow-age tables, geography, forcing and output maps, run
 * reservations and series, shortwave mode and record times, options and graphs stay with the driver, which sets them up as at
 * start-up.  Restart order: create, parameters and tables, geography and maps, shortwave mode, history entries, elmk_restart_load,
 * then the current forcing records or run series and their record times.
 * Graphs captured before a load stay valid (the arena and the history table do not move). */
enum { ELMK_CLASS_PROGNOSTIC = 0, ELMK_CLASS_SURFACE = 1, ELMK_CLASS_FORCING = 2, ELMK_CLASS_DIAGNOSTIC = 3 };
enum { ELMK_RESTART_FIELD = 0, ELMK_RESTART_HISTORY = 1, ELMK_RESTART_GRIDDED = 2, ELMK_RESTART_ACCUM = 3, ELMK_RESTART_ALT = 4,
       ELMK_RESTART_HYDROLOGY = 5, ELMK_RESTART_IRRIGATION = 6 };
enum { ELMK_RESTART_ROUTING = 7, ELMK_RESTART_IRRSUP = 8 }; /* the cell sections of version 6 */
#define ELMK_RESTART_MAGIC "ELMKRST\0"
#define ELMK_RESTART_VERSION 1u       /* of a context without accumulator entries */
#define ELMK_RESTART_VERSION_ACCUM 2u /* of a context with accumulator entries */
#define ELMK_RESTART_VERSION_ALT 3u   /* of a context with the active layer thickness enabled */
#define ELMK_RESTART_VERSION_HYDROLOGY 4u /* of a context with the soil hydrology enabled */
#define ELMK_RESTART_VERSION_IRRIGATION 5u /* of a context with the irrigation enabled */
enum { ELMK_RESTART_VERSION_ROUTING = 6 };  /* of a context with the routing enabled and ELMK_OPT_RESTART_CELLS on */
enum { ELMK_RESTART_VERSION_RESERVOIR = 7 };  /* ... and the reservoirs on: version 6 plus the cell sections ELMK_ROUTE_RES and ELMK_ROUTE_KRLS after WF */
enum { ELMK_RESTART_VERSION_HEAT = 8 };  /* ... and the stream temperature on: version 6 plus the cell sections ELMK_ROUTE_TT and ELMK_ROUTE_TR after WT */
typedef struct {
  char magic[8];              /* ELMK_RESTART_MAGIC */
  uint32_t version;           /* ELMK_RESTART_VERSION */
  uint32_t real_bytes;        /* elmk_state_real_bytes of the build that saved it */
  uint64_t schema_hash;
  int64_t gcol0, ncols;       /* global columns [gcol0, gcol0 + ncols) */
  uint64_t tape_count[4];     /* samples of each tape (ELMK_HIST_MAX_TAPES) */
  uint32_t nentries, nsections;
  uint64_t header_bytes;      /* offset of the first section */
  uint64_t total_bytes;       /* = elmk_restart_size */
  uint64_t header_checksum;
} elmk_restart_header;        /* 104 bytes */
typedef struct {
  int32_t tape, field, op, gridded; /* gridded: 1 for elmk_gridded_history_add */
  int64_t ncells;                   /* the output grid's cells for a gridded entry, else 0 */
} elmk_restart_entry;               /* 24 bytes */
typedef struct {
  int32_t kind, id, nlev, dtype;    /* ELMK_RESTART_*, field id or entry index, levels, elmk_dtype */
  int64_t extent;                   /* elements per level */
  uint64_t offset, checksum;
} elmk_restart_section;             /* 40 bytes */
typedef struct {
  int32_t src_field, kind, dst_field, pad; /* dst_field -1: none; pad 0 */
  int64_t period;
  uint64_t nsteps;                  /* the updates folded in so far */
} elmk_restart_accum;               /* 32 bytes (version 2) */
int elmk_field_class(int field);
int elmk_restart_size(elmk_ctx *ctx, int64_t *bytes);
int elmk_restart_save(elmk_ctx *ctx, int64_t gcol0, void *image, int64_t bytes);
int elmk_restart_load(elmk_ctx *ctx, int64_t gcol0, const void *image, int64_t bytes);

/* ---- the physics wrappers (same names, order and arguments as driver/kokkos) ---------------- */
int elmk_frac_wet(elmk_ctx *ctx);
int elmk_albedo_snicar(elmk_ctx *ctx);
int elmk_canopy_hydrology(elmk_ctx *ctx, double dt);
int elmk_surface_radiation(elmk_ctx *ctx);
int elmk_canopy_temperature(elmk_ctx *ctx);
int elmk_bareground_fluxes(elmk_ctx *ctx);
int elmk_canopy_fluxes(elmk_ctx *ctx, double dt);
/* L2-level forms of the two flux wrappers: the forcing-derived scalars air density / O2 / CO2 partial pressure (per column,
 * host arrays of ncols doubles; NULL = derive it as the wrapper does, canopy_fluxes_kokkos.cc:47-49 /
 * bareground_fluxes_kokkos.cc:31) handed in, which is how the reference's unit tests drive the physics with the values ELM
 * itself used (test/test_CanFlux.cc, test/test_BGFlux.cc).  Everything else as elmk_canopy_fluxes / elmk_bareground_fluxes. */
int elmk_canopy_fluxes_given(elmk_ctx *ctx, double dt, const double *forc_rho, const double *forc_po2, const double *forc_pco2);
int elmk_bareground_fluxes_given(elmk_ctx *ctx, const double *forc_rho);
int elmk_timestep7(elmk_ctx *ctx, double dt);
/* The same seven calls (elm_kokkos_interface.cc:289-307) with the five streaming wrappers between albedo and the
 * leaf-temperature iteration - canopy_hydrology, surface_radiation, canopy_temperature, the streaming stage of
 * bareground_fluxes and canopy_fluxes' initialize_flux - fused into ONE pass per column: every state element the step
 * touches is read once and written once (3 405 B per column-step instead of 5 281; BASELINE.json
 * config 5's launch structure, fp64 state).  Results are bit-identical to elmk_timestep7 in every field.  elmk_set_graph
 * applies to it as well. */
int elmk_timestep7_fused(elmk_ctx *ctx, double dt);
/* next in ELMInterface::advance (elm_kokkos_interface.cc:310): kokkos_soil_temperature(S, dt),
 * soil_temperature_kokkos.cc:6-278 - thermal properties, the 21-row pentadiagonal temperature system of
 * snow / standing surface water / soil, its solve, phase change, ground temperature */
int elmk_soil_temperature(elmk_ctx *ctx, double dt);
/* kokkos_snow_hydrology(S, dt, time_plus_half_dt) (snow_hydrology_kokkos.cc:23-188; elm_kokkos_interface.cc:313, between
 * soil_temperature and surface_fluxes; the date argument is unused by the reference's wrapper): snow_water,
 * compute_aerosol_deposition, aerosol_phase_change, transpiration, snow_compaction, combine_layers, divide_layers,
 * prune_snow_layers, update_aerosol_mass_and_concen, snow_aging - five launches in the reference, one pass per column here.
 * Updates snl and the snow mesh (dz, zsoi, zisoi, t_soisno, h2osoi_ice/liq of the snow levels and of the top soil level),
 * snw_rds, the aerosol masses mss_* and concentrations cnc_*, h2osno, snow_depth, frac_sno(_eff), int_snow, qflx_snow_melt,
 * qflx_top_soil, qflx_sl_top_soil, qflx_snow2topsoi, mflx_*, qflx_rootsoi.  The reference has no fixture for this path; the
 * checker behind the parity tests is pinned bit for bit by the reference's own snow_hydrology.h for every function
 * but the two aerosol bookkeeping functions (those: parity unpinned).  See ELMK_WARN_SNOW_* for the two
 * places where the reference's own result is undefined. */
int elmk_snow_hydrology(elmk_ctx *ctx, double dt);
/* kokkos_surface_fluxes(S, dt) (surface_fluxes_kokkos.cc:5-107): flux corrections for the new ground temperature,
 * ground heat flux, total fluxes, dew / sublimation partition, outgoing longwave, soil energy balance */
int elmk_surface_fluxes(elmk_ctx *ctx, double dt);
/* the per-column kernel at the end of kokkos_init_timestep (init_timestep_kokkos.cc:55-75): h2osno_old,
 * dtbegin_column_h2o (what the conservation check starts from), snow capping flag, frac_veg_nosno, frac_iceold.
 * (The forcing / phenology readers before it in that wrapper are I/O and stay with the caller.) */
int elmk_init_timestep(elmk_ctx *ctx);
/* The "init functions" lambda ELM::initialize_kokkos_elm runs once per column after the input files are read
 * (driver/kokkos/initialize_elm_kokkos.cc:373-428): init_topo_slope / init_melt_factor / init_micro_sigma, init_snow_layers,
 * init_soil_hydraulics, init_vegrootfr, init_soil_temp, init_snow_state, init_soilh2o_state - the producer of the state the
 * physics calls consume.  Inputs: the fields topo_slope, topo_std, snow_depth, vtype, zsoi / zisoi / dz of the soil levels
 * and the surface-data soil texture pct_sand, pct_clay, organic (by soil level; wrapper-local Views in the reference,
 * :309-311), plus elmk_set_init_params: organic_max of the parameter file (:312) and PFTData::roota_par / rootb_par [25]
 * (pft_data.h:72-73).  Writes topo_slope, n_melt, micro_sigma, snl, dz / zsoi / zisoi of the snow levels, watsat, bsw, sucsat,
 * watdry, watopt, watfc, tkmg, tkdry, csol, rootfr, t_soisno, t_grnd, h2osno, int_snow, snow_depth, h2osfc, h2ocan,
 * frac_h2osfc, fwet, fdry, frac_sno, snw_rds, h2osoi_vol, h2osoi_liq, h2osoi_ice. */
int elmk_set_init_params(elmk_ctx *ctx, double organic_max, const double *roota_par, const double *rootb_par);
int elmk_initialize_state(elmk_ctx *ctx);
/* get_forcing (driver/kokkos/atm_forcing_kokkos.cc:47-75), called by kokkos_init_timestep (init_timestep_kokkos.cc:47):
 * the eight ComputeAtmForcing_* functors of src/physics/atm_physics_impl.hh:27-203 - TBOT, PBOT, QBOT|RH, FLDS, FSDS,
 * PREC, WIND, ZBOT - over the fields atm_tbot .. atm_wind (level 0 = forcing record t_idx, level 1 = t_idx + 1 of
 * AtmDataManager::data; upload `data + t_idx * ncells` with ELMK_LAYOUT_SOA) and coszen.  Writes forc_tbot, forc_thbot,
 * forc_pbot, forc_qbot, forc_lwrad, forc_solad, forc_solai, forc_rain, forc_snow, forc_u, forc_v, forc_hgt,
 * forc_hgt_{u,t,q}_patch.  wt1, wt2: [8] host doubles in that stream order = AtmDataManager::forcing_time_weights
 * (src/data/atm_data_impl.hh:191-199) of each stream (ignored for FSDS, PREC, ZBOT); qbot_is_rh != 0: the humidity
 * stream holds relative humidity in per cent (AtmForcType::RH).  Picking t_idx and the weights is date arithmetic on
 * the host (forc_t_idx_check_bounds, atm_data_impl.hh:147-169) and stays with the caller, as do the file readers. */
int elmk_get_forcing(elmk_ctx *ctx, const double *wt1, const double *wt2, int qbot_is_rh);
/* ComputePhenology (src/physics/phenology_physics_impl.hh:22-69), run by update_phenology (phenology_kokkos.cc:59-62,
 * called at init_timestep_kokkos.cc:43) over the fields mlai, msai, mhtop, mhbot (level 0 = month start_idx, level 1 =
 * start_idx + 1 of PhenologyDataManager).  Writes tlai, tsai, htop, hbot, elai, esai, frac_veg_nosno_alb. */
int elmk_phenology(elmk_ctx *ctx, double wt1, double wt2);
/* kokkos_evaluate_conservation(S, dt) (conserved_quantity_kokkos.cc:8-81).  The reference keeps its eight
 * diagnostics in wrapper-local Views and prints column 0; here min_max_sum[8][3] receives (min, max, sum) over the
 * context's columns of dtend_column_h2o, errh2o, errh2osno, dwb, errsol, errlon, errseb, netrad - what a multi-GPU
 * run all-reduces with MIN / MAX / SUM (the reference's min_max_sum, src/utils/min_max_sum.hh:57-66) - and
 * per_column (may be NULL) the values themselves, [8][ncols].  Synchronises.
 *   Order of the sum.  The sum is a fixed function of the column values, as reduce_min_max_sum (elmkernels_amd/diagnostics.py)
 *   restates it: T = 512 x 256 threads; thread g adds x[g], x[g + T], x[g + 2T], .. in that order to +0.0; each block of 256
 *   consecutive threads then combines a[t] += a[t + s] for s = 128, 64, .., 1; one block does the same over the 512 block results
 *   (thread j adds results j and j + 256 to +0.0, then the same tree).  The same columns give the same bits on every call, in a
 *   run's rows, with and without a graph and after a restart; the bits depend on ncols (how a domain is split over contexts).
 *   Non-finite values.  If any column's value of a diagnostic is NaN, that diagnostic's min, max and sum are all NaN: a NaN sticks,
 *   as in the history tapes.  +inf and -inf are ordinary values (min = -inf, max = +inf; both among the columns give sum = NaN).
 *   The sign of a min or max that is zero is unspecified. */
int elmk_evaluate_conservation(elmk_ctx *ctx, double dt, double *min_max_sum, double *per_column);
/* Everything ELMInterface::advance calls per column after kokkos_init_timestep, in its order
 * (elm_kokkos_interface.cc:289-316): the seven wrappers (as elmk_timestep7_fused), kokkos_soil_temperature,
 * kokkos_snow_hydrology, kokkos_surface_fluxes - one call, and with elmk_set_graph one HIP graph launch per model step.
 * Same bits as the ten calls.  elmk_set_snow_age_tables must have been called.  (kokkos_evaluate_conservation returns
 * values to the host and stays a call of its own.) */
int elmk_advance_physics(elmk_ctx *ctx, double dt);

/* ---- diagnostics ---------------------------------------------------------------------------- */
/* OR of all columns' flag words and the first column with a fatal bit (-1 if none); synchronises */
int elmk_error_summary(elmk_ctx *ctx, uint32_t *or_of_flags, int64_t *first_bad_col);
int elmk_clear_errors(elmk_ctx *ctx);
/* run `nsteps` timesteps with HIP events between the seven launches on the context's stream;
 * ms_per_kernel[7] (frac_wet, albedo_snicar, canopy_hydrology, surface_radiation, canopy_temperature,
 * bareground_fluxes, canopy_fluxes) receives the mean device time of each launch, *ms_total the mean
 * time of one whole timestep (first event to last).  If a snapshot exists (elmk_snapshot_fields) it is
 * restored before every step, outside the event brackets, so each profiled step does the same work. */
int elmk_profile_timestep7(elmk_ctx *ctx, double dt, int nsteps, float *ms_per_kernel, float *ms_total);
/* the same for elmk_timestep7_fused: ms_per_stage[5] = frac_wet + list resets + queue class count (k_fz_prep);
 * albedo_snicar; the fused streaming pass (k_fz_stream); the bare-ground flux list; the leaf-temperature iteration +
 * compute_flux (k_cf_iterate, k_cf_finish) */
int elmk_profile_timestep7_fused(elmk_ctx *ctx, double dt, int nsteps, float *ms_per_stage, float *ms_total);
/* the same for one wrapper: mean device time over nsteps launches, HIP events on the context's stream, the snapshot (if
 * any) restored before every launch outside the event brackets */
typedef enum {
  ELMK_WRAPPER_FRAC_WET = 0, ELMK_WRAPPER_ALBEDO_SNICAR, ELMK_WRAPPER_CANOPY_HYDROLOGY, ELMK_WRAPPER_SURFACE_RADIATION,
  ELMK_WRAPPER_CANOPY_TEMPERATURE, ELMK_WRAPPER_BAREGROUND_FLUXES, ELMK_WRAPPER_CANOPY_FLUXES,
  ELMK_WRAPPER_SOIL_TEMPERATURE, ELMK_WRAPPER_SURFACE_FLUXES, ELMK_WRAPPER_SNOW_HYDROLOGY,
  ELMK_WRAPPER_ADVANCE_PHYSICS /* elmk_advance_physics: all ten in the reference's order */
} elmk_wrapper;
int elmk_profile_wrapper(elmk_ctx *ctx, int wrapper, double dt, int nsteps, float *ms_mean);
/* device time of each of nsteps steps of elmk_timestep7 (fused = 0) or elmk_timestep7_fused (fused != 0), by HIP events
 * around every step on the context's stream, the snapshot restored before every step outside the brackets: what the
 * benchmark takes its median step time from */
int elmk_profile_steps(elmk_ctx *ctx, int fused, double dt, int nsteps, float *ms_each_step);
/* Read back context-owned scratch (diagnostics; not part of the state contract).
 *   ELMK_SCRATCH_CF_TRIPS: int32 per column - trips of the leaf-temperature iteration
 *                          (canopy_fluxes_impl.hh:233-450) in the last elmk_canopy_fluxes call, 0 = not vegetated
 *   ELMK_SCRATCH_WORK:     doubles of the work arrays, raw (development probes)
 * Synchronises the stream. */
enum {
  ELMK_SCRATCH_CF_TRIPS = 0,
  ELMK_SCRATCH_WORK = 1,
  ELMK_SCRATCH_CF_HINTS = 2,   /* int32 per column: the scheduling hint (decaying maximum of the trip count) */
  ELMK_SCRATCH_LIST_COUNTS = 3 /* uint32 x 2 per internal work list: entries, queue head.  Every list is left empty by the
                                  wrapper that filled it, so both read 0 between two calls (a test asserts it) */
};
int elmk_read_scratch(elmk_ctx *ctx, int kind, void *host, int64_t offset, int64_t count);
/* device-to-device copy bandwidth probe (read+write bytes / s) on this context's device, used as the
 * empirical HBM line next to the 8 TB/s datasheet peak */
int elmk_copy_bandwidth(elmk_ctx *ctx, int64_t bytes, int iters, double *gbytes_per_s);
/* the same probe in a chosen access shape: 0 = 8 bytes per lane, one load per thread (the shape of elmk_copy_bandwidth and of
 * the snapshot restore); 1 = 16 bytes per lane; 2 = 8 bytes per lane, four independent loads per thread; 3 = 16 bytes per
 * lane, four independent loads per thread; 4 = 8 bytes per lane, 64 separate streams read and 64 written by every thread
 * (the buffer seen as 64 fields, field-major like the state).  bench.py reports the best of 0..3 as roofline.empirical_peak
 * and shape 4 as the line of a many-field streaming kernel. */
int elmk_copy_bandwidth_shape(elmk_ctx *ctx, int64_t bytes, int iters, int shape, double *gbytes_per_s);
/* Evaluate one function of elmkernels_amd/csrc/elmk_math.h - the device restatement of the host libm's exp / log / log10 /
 * pow / atan / tanh / cos / erf / acos / expm1 / sin (the <cmath> calls of src/physics headers and of incident_shortwave.cc) - on n host values: out[i] = fn(x[i]) or pow(x[i], y[i]).
 * ELMK_MATH_SQRT and ELMK_MATH_DIV (x[i] / y[i]) are the device's own IEEE operations, included so that the tests can
 * confirm they round correctly.  y is read only for ELMK_MATH_POW / ELMK_MATH_DIV.  Used by the parity tests to compare the device bits with the host libm's. */
typedef enum {
  ELMK_MATH_EXP = 0, ELMK_MATH_LOG, ELMK_MATH_LOG10, ELMK_MATH_ATAN, ELMK_MATH_SQRT, ELMK_MATH_TANH, ELMK_MATH_COS, ELMK_MATH_ERF,
  ELMK_MATH_ACOS, ELMK_MATH_EXPM1, ELMK_MATH_DIV, ELMK_MATH_POW,
  ELMK_MATH_SIN /* (appended: the ids above do not move) */
} elmk_math_fn;
int elmk_math_eval(elmk_ctx *ctx, int fn, const double *x, const double *y, double *out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif /* ELMK_H */
