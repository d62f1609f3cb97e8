// api_run.cpp - multi-step runs and what feeds them: the series, the forcing grid, aerosol deposition, shortwave COSZEN mode and
// downscaling (include/elmk.h "multi-step runs", "forcing grid", "aerosol deposition", "shortwave", "downscaling").
#include "elmk_ctx.h"

namespace {
// quiesce and release the reservation: elmk_run_reserve, elmk_set_forcing_grid and elmk_clear_forcing_grid
int run_drop(elmk_ctx* ctx)
{
  if (int rc = quiesce(ctx, true)) return rc;
  ctx->run = elmk_ctx::Run{};
  return wb_ring_alloc(ctx);  // (frees the water balance's ring rows of the reservation)
}

// the internal copy stream of elmk_series_upload and elmk_aerosol_upload, with the events of the two run buffers
int ensure_upload_stream(elmk_ctx* ctx)
{
  if (ctx->upload) return ELMK_OK;
  HIPCHK(hipStreamCreateWithFlags(&ctx->upload, hipStreamNonBlocking));
  for (int b = 0; b < 2; b++) {
    HIPCHK(hipEventCreateWithFlags(&ctx->run_done[b], hipEventDisableTiming));
  }
  return ELMK_OK;
}

void run_solar_geometry(elmk_ctx* ctx, double)
{
  if (ctx->sw.mode == ELMK_SW_COSZEN)
    launch_solar_geometry_run_cz(ctx->d, ctx->ncols, ctx->run.table, ctx->run.cursor, ctx->run.rec, ctx->sw.czf, ctx->stream);
  else
    launch_solar_geometry_run(ctx->d, ctx->ncols, ctx->run.table, ctx->run.cursor, ctx->stream);
}
void run_phenology(elmk_ctx* ctx, double) { launch_phenology_run(ctx->d, ctx->ncols, ctx->run.table, ctx->run.cursor, ctx->run.phen, ctx->stream); }
void run_forcing(elmk_ctx* ctx, double)
{
  const elmk_ctx::Run& R = ctx->run;
  const EllMap& G = ctx->grid.map;
  const double* czf = ctx->sw.mode == ELMK_SW_COSZEN ? (const double*)ctx->sw.czf : nullptr;
  const DsParams P = ds_params(ctx);
  const DsParams* ds = ds_topo(ctx) ? &P : nullptr;
  if (ctx->grid.mem)
    launch_get_forcing_run_grid(ctx->d, ctx->ncols, R.table, R.cursor, R.forc, R.slots, R.fstride, G.npad, G.idx, G.w,
                                (R.flags & ELMK_RUN_QBOT_IS_RH) != 0, ctx->stream, czf, ds);
  else
    launch_get_forcing_run(ctx->d, ctx->ncols, R.table, R.cursor, R.forc, R.slots, (R.flags & ELMK_RUN_QBOT_IS_RH) != 0, ctx->stream, czf, ds);
  ds_lw_norm(ctx);
}
AerSeries aer_series(const elmk_ctx* ctx)
{
  const elmk_ctx::Aerosol& A = ctx->aer;
  return AerSeries{A.cells, A.map.ncells, A.map.npad, A.map.idx, A.map.w};
}
void run_aerosol(elmk_ctx* ctx, double)
{
  if (ctx->run.flags & ELMK_RUN_AEROSOL)
    launch_aerosol_deposition_run(ctx->d, ctx->ncols, aer_series(ctx), ctx->run.table, ctx->run.cursor, ctx->stream);
}
void run_init_timestep(elmk_ctx* ctx, double) { launch_init_timestep(ctx->d, ctx->ncols, ctx->stream); }
void run_wb_begin(elmk_ctx* ctx, double)
{
  if (ctx->run.flags & ELMK_RUN_WATER_BALANCE) wb_begin_launch(ctx);
}
void run_water_balance(elmk_ctx* ctx, double dt)
{
  if (ctx->run.flags & ELMK_RUN_WATER_BALANCE) wb_launch(ctx, dt, true);
}
void run_soil_hydrology(elmk_ctx* ctx, double dt)
{
  if (ctx->run.flags & ELMK_RUN_HYDROLOGY) hyd_launch(ctx, dt);
}
void run_conservation(elmk_ctx* ctx, double dt)
{
  const elmk_ctx::Run& R = ctx->run;
  launch_conservation_run(ctx->d, ctx->ncols, ctx->ld, dt, ELMK_GENERIC(ctx->h.cons_diag), ctx->cons_part, R.cons, R.flag_or,
                          R.flag_first, R.cursor, ctx->stream);
}
void run_flag_reduce(elmk_ctx* ctx, double)
{
  const elmk_ctx::Run& R = ctx->run;
  launch_flag_reduce_run((const uint32_t*)ctx->fptr[ELMK_FIELD_err_flags], ctx->ncols, R.flag_or, R.flag_first, R.cursor, ctx->stream);
}
void run_routing(elmk_ctx* ctx, double dt)
{
  if (ctx->run.flags & ELMK_RUN_ROUTING) route_launch(ctx, dt, true);
}
void run_active_layer(elmk_ctx* ctx, double)
{
  if (ctx->run.flags & ELMK_RUN_ALT) launch_active_layer_run(alt_args(ctx), ctx->run.table, ctx->run.cursor, ctx->stream);
}
void run_accum(elmk_ctx* ctx, double)
{
  if (ctx->run.flags & ELMK_RUN_ACCUM) accum_update_launch(ctx);
}
void run_history(elmk_ctx* ctx, double)
{
  if ((ctx->run.flags & ELMK_RUN_HISTORY) && !ctx->hist.empty()) hist_accumulate_launch(ctx);
}
void run_points(elmk_ctx* ctx, double)
{
  if (ctx->pts.run_on) points_run_launch(ctx);
}
void run_next(elmk_ctx* ctx, double) { launch_run_next(ctx->run.cursor, ctx->stream); }

bool aerosol_field(int f) { return f >= ELMK_FIELD_aer_bcphi && f <= ELMK_FIELD_aer_dst4_2; }
bool rec_decday_ok(double d) { return d >= 0.0 && d < 1.0e9; }
int ds_alloc_topo(elmk_ctx* ctx)
{
  elmk_ctx::Downscale& D = ctx->ds;
  if (D.topo) return ELMK_OK;
  const size_t bytes = 2 * (size_t)ctx->ld * sizeof(double);
  if (hip_fail(ctx, D.topo.alloc(bytes), "hipMalloc(elevations)")) return ELMK_E_NOMEM;
  HIPCHK(hipMemsetAsync(D.topo, 0, bytes, ctx->stream));
  return ELMK_OK;
}
bool all_finite(const double* a, int64_t n)
{
  for (int64_t i = 0; i < n; i++)
    if (!std::isfinite(a[i])) return false;
  return true;
}

// one model step of elmk_run, in the order of the stand-alone calls it replaces (include/elmk.h): solar geometry, phenology,
// forcing, aerosol deposition (ELMK_RUN_AEROSOL: where the reference's hook sits, init_timestep_kokkos.cc:48-49), init_timestep,
// the water balance's begin (ELMK_RUN_WATER_BALANCE), advance_physics' stages (one stage here: launch_advance, with the irrigation stage
// in front of soil_temperature under ELMK_RUN_IRRIGATION), soil hydrology
// (ELMK_RUN_HYDROLOGY), conservation -> ring row, flag summary -> ring row, water balance -> its ring rows, runoff routing
// (ELMK_RUN_ROUTING), active layer thickness (ELMK_RUN_ALT), accumulated fields, history, the point series' record (while
// elmk_points_set_run is in force), next row
constexpr Stage RUN_STEP[] = {{run_solar_geometry, nullptr}, {run_phenology, nullptr},     {run_forcing, nullptr},        {run_aerosol, nullptr},
                              {run_init_timestep, nullptr},  {run_wb_begin, nullptr},      {launch_advance, nullptr},     {run_soil_hydrology, nullptr},
                              {run_conservation, nullptr},   {run_flag_reduce, nullptr},   {run_water_balance, nullptr},  {run_routing, nullptr},
                              {run_active_layer, nullptr},   {run_accum, nullptr},         {run_history, nullptr},        {run_points, nullptr},
                              {run_next, nullptr}};
}  // namespace

namespace elmk {

DsParams ds_params(const elmk_ctx* ctx)
{
  const elmk_ctx::Downscale& D = ctx->ds;
  return DsParams{D.topo, D.topo + ctx->ld, D.gmem ? D.lg : nullptr, D.lapse, D.lapse_lw, D.lw_limit};
}
// after a TOPO forcing kernel while groups are set: the longwave renormalisation over the groups
void ds_lw_norm(elmk_ctx* ctx)
{
  const elmk_ctx::Downscale& D = ctx->ds;
  const CsrMap& G = D.groups;
  if (!ds_topo(ctx) || !D.gmem) return;
  launch_ds_lw_norm(ctx->fptr[ELMK_FIELD_forc_lwrad], store_dtype(ELMK_F64), D.lg, OGridMap{G.ptr, G.col, G.w, G.nrows, 0.0}, D.wsum, ctx->stream);
}

int sw_reset(elmk_ctx* ctx, int mode, double forc_dt)
{
  if (int rc = quiesce(ctx, false)) return rc;
  elmk_ctx::Shortwave& W = ctx->sw;
  W.mode = mode;
  W.forc_dt = mode == ELMK_SW_COSZEN ? forc_dt : 0.0;
  W.step_time = W.czf_ready = false;
  std::fill(ctx->run.rec_set.begin(), ctx->run.rec_set.end(), 0);
  return ELMK_OK;
}
}  // namespace elmk

extern "C" {

// ---------------------------------------------------------------------------------------------------
// multi-step runs: the driver's time loop (kokkos_driver.cc:54-85) on the device
// ---------------------------------------------------------------------------------------------------
int elmk_run_reserve(elmk_ctx* ctx, int forcing_slots, int max_steps)
{
  if (int rc = enter(ctx)) return rc;
  if (forcing_slots < 2 || forcing_slots > (1 << 20) || max_steps < 1 || max_steps > (1 << 24))
    return invalid(ctx, "elmk_run_reserve: need 2 <= forcing_slots <= 2^20 and 1 <= max_steps <= 2^24");
  if (int rc = refuse_capture(ctx, "elmk_run_reserve")) return rc;
  elmk_ctx::Run& R = ctx->run;
  if (int rc = run_drop(ctx)) return rc;
  if (int rc = ensure_upload_stream(ctx)) return rc;
  const size_t es = (size_t)store_size(ELMK_F64), ld = (size_t)ctx->ld, nrow = 2 * (size_t)max_steps;
  // with a forcing grid the forcing records are cell records, [RUN_NFORC][slots][ncells] without padding
  const int64_t fstride = ctx->grid.mem ? ctx->grid.map.ncells : ctx->ld;
  if (hip_fail(ctx, carve(R.mem, [&](Carve& L) {
                 L.take(R.forc, (size_t)RUN_NFORC * forcing_slots * (size_t)fstride * es);
                 L.take(R.phen, (size_t)RUN_NPHEN * RUN_NMONTH * ld * es);
                 L.take(R.table, nrow * sizeof(RunRow));
                 L.take(R.cursor, 256);
                 L.take(R.cons, nrow * 24 * sizeof(double));
                 L.take(R.flag_or, nrow * sizeof(uint32_t));
                 L.take(R.flag_first, nrow * sizeof(long long));
               }), "hipMalloc(run)"))
    return ELMK_E_NOMEM;
  if (hip_fail(ctx, R.rows.alloc(nrow * sizeof(RunRow)), "hipHostMalloc(run steps)")) {
    R = elmk_ctx::Run{};
    return ELMK_E_NOMEM;
  }
  R.slots = forcing_slots;
  R.max_steps = max_steps;
  R.fcols = ctx->grid.mem ? ctx->grid.map.ncells : ctx->ncols;
  R.fstride = fstride;
  if (hip_fail(ctx, hipMemsetAsync(R.mem, 0, R.mem.bytes(), ctx->stream), "hipMemset(run)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    R = elmk_ctx::Run{};
    return ELMK_E_HIP;
  }
  if (int rc = wb_ring_alloc(ctx)) {
    R = elmk_ctx::Run{};
    return rc;
  }
  return ELMK_OK;
}

int elmk_series_upload(elmk_ctx* ctx, int field, int slot0, int nslots, const double* host, int64_t col0, int64_t n)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Run& R = ctx->run;
  if (!R.mem) return invalid(ctx, "elmk_series_upload: elmk_run_reserve has not been called");
  const bool forcing = field >= ELMK_FIELD_atm_tbot && field <= ELMK_FIELD_atm_wind;
  const bool phen = field >= ELMK_FIELD_mlai && field <= ELMK_FIELD_mhbot;
  static_assert(ELMK_FIELD_atm_wind - ELMK_FIELD_atm_tbot + 1 == RUN_NFORC && ELMK_FIELD_mhbot - ELMK_FIELD_mlai + 1 == RUN_NPHEN,
                "series fields");
  if (!forcing && !phen) return invalid(ctx, "elmk_series_upload: not a series field (atm_tbot .. atm_wind, mlai .. mhbot)");
  const int k = forcing ? field - ELMK_FIELD_atm_tbot : field - ELMK_FIELD_mlai;
  const int nsl = forcing ? R.slots : RUN_NMONTH;
  if (slot0 < 0 || nslots < 0 || slot0 + (int64_t)nslots > nsl) return invalid(ctx, "elmk_series_upload: slots out of range");
  const int64_t ncol = forcing ? R.fcols : ctx->ncols, stride = forcing ? R.fstride : ctx->ld;  // (cells in grid mode)
  if ((!host && n > 0 && nslots > 0) || col0 < 0 || n < 0 || col0 + n > ncol)
    return invalid(ctx, "elmk_series_upload: bad column (grid mode: cell) range");
  if (n == 0 || nslots == 0) return ELMK_OK;
  const auto reads = [&](int b) {  // the run on buffer b reads some of these records
    return forcing ? (slot0 <= R.slot_hi[b] && slot0 + nslots - 1 >= R.slot_lo[b]) : ((R.months[b] >> slot0) & ((1u << nslots) - 1u)) != 0;
  };
  if (int rc = wait_for_runs(ctx, reads)) return rc;
  const size_t es = (size_t)store_size(ELMK_F64);
  char* dst = (forcing ? R.forc : R.phen) + (((size_t)k * nsl + slot0) * (size_t)stride + (size_t)col0) * es;
  const void* src = host;
  std::vector<float> tmp;
  if (kStateF32) {  // rounded to the stored fp32 as xfer rounds an upload
    const size_t cnt = (size_t)nslots * (size_t)n;
    tmp.resize(cnt);
    for (size_t i = 0; i < cnt; i++) tmp[i] = (float)host[i];
    src = tmp.data();
  }
  HIPCHK(hipMemcpy2DAsync(dst, (size_t)stride * es, src, (size_t)n * es, (size_t)n * es, (size_t)nslots, hipMemcpyHostToDevice, ctx->upload));
  HIPCHK(hipStreamSynchronize(ctx->upload));  // (caller's pageable source; a run enqueued after this call sees the records)
  return ELMK_OK;
}

int elmk_run(elmk_ctx* ctx, double dt, const elmk_run_step* steps, int nsteps, int flags)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Run& R = ctx->run;
  // every refusal before anything is enqueued
  if (!R.mem) return invalid(ctx, "elmk_run: elmk_run_reserve has not been called");
  if (!ctx->geo_set) return invalid(ctx, "elmk_run: no column geography (elmk_set_column_geography)");
  if (!ctx->snowage_set) return invalid(ctx, "elmk_run: the snow-age tables are not set (elmk_set_snow_age_tables)");
  if (nsteps < 1 || nsteps > R.max_steps || !steps) return invalid(ctx, "elmk_run: nsteps outside 1 .. max_steps of elmk_run_reserve");
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_run: dt must be finite and positive");
  if (flags & ~(ELMK_RUN_QBOT_IS_RH | ELMK_RUN_HISTORY | ELMK_RUN_ACCUM | ELMK_RUN_AEROSOL | ELMK_RUN_ALT | ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE |
                ELMK_RUN_IRRIGATION | ELMK_RUN_ROUTING))
    return invalid(ctx, "elmk_run: unknown flags");
  if ((flags & ELMK_RUN_AEROSOL) && !ctx->aer.mem) return invalid(ctx, "elmk_run: ELMK_RUN_AEROSOL without an aerosol series (elmk_aerosol_reserve)");
  if ((flags & ELMK_RUN_ACCUM) && ctx->accum.empty()) return invalid(ctx, "elmk_run: ELMK_RUN_ACCUM without an accumulator entry (elmk_accum_add)");
  if ((flags & ELMK_RUN_ALT) && !ctx->alt_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_ALT without the active layer thickness enabled (elmk_active_layer_enable)");
  if ((flags & ELMK_RUN_HYDROLOGY) && !ctx->hyd_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_HYDROLOGY without the soil hydrology enabled (elmk_soil_hydrology_enable)");
  if ((flags & ELMK_RUN_HYDROLOGY) && !ctx->hyd_params)
    return invalid(ctx, "elmk_run: ELMK_RUN_HYDROLOGY without parameters (elmk_soil_hydrology_set_params)");
  if ((flags & ELMK_RUN_WATER_BALANCE) && !ctx->wb_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_WATER_BALANCE without the water balance enabled (elmk_water_balance_enable)");
  if ((flags & ELMK_RUN_WATER_BALANCE) && !(flags & ELMK_RUN_HYDROLOGY))
    return invalid(ctx, "elmk_run: ELMK_RUN_WATER_BALANCE without ELMK_RUN_HYDROLOGY");
  if ((flags & ELMK_RUN_IRRIGATION) && !ctx->irr_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_IRRIGATION without the irrigation enabled (elmk_irrigation_enable)");
  if ((flags & ELMK_RUN_IRRIGATION) && !(dt >= 1.0 && dt <= 86400.0 && dt == std::floor(dt)))
    return invalid(ctx, "elmk_run: ELMK_RUN_IRRIGATION needs dt to be a whole number of seconds in 1 .. 86400");
  if ((flags & ELMK_RUN_ROUTING) && !ctx->route.mem)
    return invalid(ctx, "elmk_run: ELMK_RUN_ROUTING without the runoff routing enabled (elmk_routing_enable)");
  if ((flags & ELMK_RUN_ROUTING) && !(flags & ELMK_RUN_WATER_BALANCE))
    return invalid(ctx, "elmk_run: ELMK_RUN_ROUTING without ELMK_RUN_WATER_BALANCE");
  const bool cz = ctx->sw.mode == ELMK_SW_COSZEN;
  int lo = R.slots, hi = -1;
  unsigned months = 0;
  for (int s = 0; s < nsteps; s++) {
    const elmk_run_step& p = steps[s];
    if (p.forc_slot < 0 || p.forc_slot > R.slots - 2) return invalid(ctx, "elmk_run: forc_slot outside 0 .. forcing_slots - 2");
    if (cz && !(R.rec && R.rec_set[p.forc_slot]))
      return invalid(ctx, "elmk_run: shortwave COSZEN mode: a step's forc_slot has no record time (elmk_series_record_times)");
    if (p.month1 < 0 || p.month1 >= RUN_NMONTH || p.month2 < 0 || p.month2 >= RUN_NMONTH) return invalid(ctx, "elmk_run: month outside 0 .. 11");
    if (!(p.decday >= 0.0 && p.decday < 1.0e9) || p.doy < -1 || p.doy > 1000000000) return invalid(ctx, "elmk_run: bad decday / doy");
    lo = std::min(lo, (int)p.forc_slot);
    hi = std::max(hi, (int)p.forc_slot + 1);
    months |= (1u << p.month1) | (1u << p.month2);
  }
  if (int rc = points_run_check(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_run")) return rc;

  if (int rc = set_col_dayl(ctx, true)) return rc;  // per-column mode, as the first elmk_solar_geometry enters it
  if (int rc = heal_lists(ctx)) return rc;
  if (int rc = push_params(ctx)) return rc;
  // this buffer was last used by run count - 2: wait for its end before its pinned rows, device table, ring rows and read set are
  // reused (otherwise an upload after this call would no longer know that run's read set and could write under it)
  const int buf = (int)(R.count & 1);
  if (R.live[buf]) HIPCHK(hipEventSynchronize(ctx->run_done[buf]));
  RunRow* rows = R.rows + (size_t)buf * R.max_steps;
  for (int s = 0; s < nsteps; s++) {
    const elmk_run_step& p = steps[s];
    RunRow& r = rows[s];
    r.sol = elmk_solar_step_consts(dt, p.decday, p.doy);
    memcpy(r.forc_wt1, p.forc_wt1, sizeof r.forc_wt1);
    memcpy(r.forc_wt2, p.forc_wt2, sizeof r.forc_wt2);
    r.month_wt1 = p.month_wt1;
    r.month_wt2 = p.month_wt2;
    r.forc_slot = p.forc_slot;
    r.month1 = p.month1;
    r.month2 = p.month2;
    // the annual rollover of the active layer thickness: the step that starts at 00:00 of 1 January (north) / 1 July (south) of the
    // no-leap calendar, whose end-of-step date satisfies ELM's mon, day == 1 && sec / dtime == 1
    r.pad = !(flags & ELMK_RUN_ALT) ? 0
                                    : (p.doy == 0 && p.decday == 1.0 ? ELMK_ALT_ROLL_NORTH : 0) |
                                          (p.doy == 181 && p.decday == 182.0 ? ELMK_ALT_ROLL_SOUTH : 0);
    // the irrigation's time of day: seconds after midnight UTC at the step's start, above the rollover bits
    if (flags & ELMK_RUN_IRRIGATION) {
      const long long t = std::llround((p.decday - 1.0 - (double)p.doy) * 86400.0);
      r.pad |= (int32_t)(((t % 86400) + 86400) % 86400) << RUN_PAD_TOD_SHIFT;
    }
    // the reservoirs' month and whether the step starts at 00:00 of its first day (the rollover's test), above the time of day
    if ((flags & ELMK_RUN_ROUTING) && ctx->route.dam.mem) {
      const int m = reservoir_month(p.doy);
      r.pad |= (int32_t)(m | (reservoir_month_begins(p.doy, p.decday) ? 16 : 0)) << RUN_PAD_DAM_SHIFT;
    }
  }
  const int row0 = buf * R.max_steps;
  HIPCHK(hipMemcpyAsync(R.table + row0, rows, (size_t)nsteps * sizeof(RunRow), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)R.cursor, row0, 1, ctx->stream));
  if (ctx->pts.run_on)
    if (int rc = points_run_begin(ctx, buf, steps, nsteps)) return rc;
  R.flags = flags;
  R.live[buf] = true;  // (from here on an upload of these records waits for the run's end event)
  R.slot_lo[buf] = lo;
  R.slot_hi[buf] = hi;
  R.months[buf] = months;
  R.aer_months[buf] = (flags & ELMK_RUN_AEROSOL) ? months : 0u;
  R.count++;
  R.last_buf = buf;
  R.last_nsteps = nsteps;
  ctx->wb_ran = (flags & ELMK_RUN_WATER_BALANCE) != 0;
  if (flags & ELMK_RUN_ROUTING) ctx->route.ncalls += nsteps;  // (the calls are enqueued below)
  ctx->wb_ran_empty = ctx->wb_ran && (!hyd_land(ctx) || ctx->ncols <= 0);
  // what the captured step depends on: the stages of the flags, modes and land unit, and the tables of their versions' moment
  const StepKey key{flags, ds_topo(ctx), ds_topo(ctx) && ctx->ds.gmem, cz, (flags & ELMK_RUN_HYDROLOGY) && hyd_land(ctx),
                    (flags & ELMK_RUN_HYDROLOGY) && (bool)ctx->hydf_rows, ctx->hist_version,
                    ctx->accum_version, (flags & ELMK_RUN_IRRIGATION) && hyd_land(ctx),
                    (flags & ELMK_RUN_WATER_BALANCE) && (bool)ctx->irr_rows, (flags & ELMK_RUN_ROUTING) && ctx->route.withdraw,
                    (flags & ELMK_RUN_IRRIGATION) && hyd_land(ctx) && (bool)ctx->irrsup_rows,
                    (flags & ELMK_RUN_ROUTING) && (bool)ctx->route.dam.mem, (flags & ELMK_RUN_ROUTING) && (bool)ctx->route.heat.mem,
                    (bool)ctx->route.land.mem, (bool)ctx->route.cmd.mem, points_key(ctx),
                    (flags & ELMK_RUN_HYDROLOGY) && hyd_land(ctx) && (bool)ctx->hs.mem};
  if (cz) {  // the run's czf replaces the stepwise record time's
    ctx->sw.step_time = false;
    ctx->sw.czf_ready = true;
  }
  int rc = ELMK_OK;
  for (int s = 0; s < nsteps && rc == ELMK_OK; s++) rc = launch_sequence(ctx, GRAPH_RUN_STEP, RUN_STEP, dt, key);
  HIPCHK(hipEventRecord(ctx->run_done[buf], ctx->stream));
  if (rc) return rc;
  if ((flags & ELMK_RUN_HISTORY) && !ctx->hist.empty()) mark_sampled(ctx, hist_tape_mask(ctx));
  return ELMK_OK;
}

int elmk_run_diagnostics(elmk_ctx* ctx, double* min_max_sum, uint32_t* flags_or, int64_t* first_bad_col)
{
  if (int rc = enter(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const elmk_ctx::Run& R = ctx->run;
  if (R.last_buf < 0) return 0;
  const size_t row0 = (size_t)R.last_buf * R.max_steps, n = (size_t)R.last_nsteps;
  std::vector<long long> f(first_bad_col ? n : 0);
  if (min_max_sum) HIPCHK(hipMemcpyAsync(min_max_sum, R.cons + row0 * 24, n * 24 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (flags_or) HIPCHK(hipMemcpyAsync(flags_or, R.flag_or + row0, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (first_bad_col) HIPCHK(hipMemcpyAsync(f.data(), R.flag_first + row0, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < f.size(); i++) first_bad_col[i] = (f[i] == 0x7fffffffffffffffll) ? -1 : (int64_t)f[i];
  return (int)n;
}

// ---------------------------------------------------------------------------------------------------
// forcing on a coarser grid: a per-column ELL remap map on the device (include/elmk.h "forcing grid")
// ---------------------------------------------------------------------------------------------------
int elmk_set_forcing_grid(elmk_ctx* ctx, int64_t ncells, int npts, const int32_t* idx, const double* w)
{
  if (int rc = enter(ctx)) return rc;
  // (every gather of the remap kernels stays inside a cell record because of this check)
  if (int rc = invalid_map(ctx, "elmk_set_forcing_grid", ell_check(ctx->ncols, ncells, npts, idx, w))) return rc;
  if (int rc = refuse_capture(ctx, "elmk_set_forcing_grid")) return rc;
  if (int rc = run_drop(ctx)) return rc;
  elmk_ctx::Grid& G = ctx->grid;
  G = elmk_ctx::Grid{};
  const int rc = hip_fail(ctx, carve(G.mem, [&](Carve& L) {
                            G.map.take(L, ncells, npts, (size_t)ctx->ld);
                            L.take(G.cells, (size_t)ncells * sizeof(double));
                          }), "hipMalloc(forcing grid)")
                     ? ELMK_E_NOMEM
                     : G.map.upload(ctx, "grid", G.mem + G.mem.bytes(), idx, w);  // (zeroes the cells behind w too)
  if (rc != ELMK_OK) G = elmk_ctx::Grid{};
  return rc;
}

int elmk_clear_forcing_grid(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_clear_forcing_grid")) return rc;
  if (int rc = run_drop(ctx)) return rc;
  ctx->grid = elmk_ctx::Grid{};
  return ELMK_OK;
}

int elmk_upload_gridded(elmk_ctx* ctx, int field, int level, const double* cells)
{
  if (int rc = enter(ctx)) return rc;
  const elmk_ctx::Grid& G = ctx->grid;
  if (!G.mem) return invalid(ctx, "elmk_upload_gridded: no forcing grid (elmk_set_forcing_grid)");
  if (!field_ok(field) || g_fields[field].dtype != ELMK_F64) return invalid(ctx, "elmk_upload_gridded: not an fp64 field");
  if (level < 0 || level >= g_fields[field].nlev) return invalid(ctx, "elmk_upload_gridded: level out of range");
  if (!cells) return invalid(ctx, "elmk_upload_gridded: null cells");
  if (int rc = refuse_capture(ctx, "elmk_upload_gridded")) return rc;
  if (ctx->ncols == 0) return ELMK_OK;
  char* dst = (char*)ctx->fptr[field] + (size_t)level * (size_t)ctx->ld * (size_t)store_size(ELMK_F64);
  // staging is reused by the next call: the copy and the remap are done when this returns, as elmk_upload's copy is
  HIPCHK(hipMemcpyAsync(G.cells, cells, (size_t)G.map.ncells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_remap_field(dst, G.cells, ctx->ncols, ctx->ld, G.map.npad, G.map.idx, G.map.w, ctx->stream);
  HIPCHK(hipGetLastError());
  return synced(ctx);
}

// ---------------------------------------------------------------------------------------------------
// aerosol deposition: a monthly climatology on a grid of its own, interpolated on the device (include/elmk.h "aerosol deposition")
// ---------------------------------------------------------------------------------------------------
int elmk_aerosol_reserve(elmk_ctx* ctx, int64_t ncells, int npts, const int32_t* idx, const double* w)
{
  if (int rc = enter(ctx)) return rc;
  if ((idx == nullptr) != (w == nullptr)) return invalid(ctx, "elmk_aerosol_reserve: idx and w must both be given or both be NULL");
  const bool mapped = idx != nullptr;
  if (ncells < 1 || ncells > INT32_MAX) return invalid(ctx, "elmk_aerosol_reserve: ncells outside 1 .. 2^31-1");
  if (!mapped && ncells != ctx->ncols) return invalid(ctx, "elmk_aerosol_reserve: without a map the series are per column: ncells must equal ncols");
  // (every gather of k_aerosol_deposition stays inside a cell record because of this check)
  if (mapped)
    if (int rc = invalid_map(ctx, "elmk_aerosol_reserve", ell_check(ctx->ncols, ncells, npts, idx, w))) return rc;
  if (int rc = refuse_capture(ctx, "elmk_aerosol_reserve")) return rc;
  if (int rc = quiesce(ctx, true)) return rc;  // (the run reservation stays)
  if (int rc = ensure_upload_stream(ctx)) return rc;
  if (!ctx->aer_step_done) HIPCHK(hipEventCreateWithFlags(&ctx->aer_step_done, hipEventDisableTiming));
  elmk_ctx::Aerosol& A = ctx->aer;
  A = elmk_ctx::Aerosol{};
  A.map.ncells = ncells;
  const size_t series_bytes = align_up((size_t)AER_NSTREAM * RUN_NMONTH * (size_t)ncells * sizeof(double), 256);
  int rc = ELMK_OK;
  if (hip_fail(ctx, carve(A.mem, [&](Carve& L) {
                 L.take(A.cells, series_bytes);
                 if (mapped) A.map.take(L, ncells, npts, (size_t)ctx->ld);
               }), "hipMalloc(aerosol series)"))
    rc = ELMK_E_NOMEM;
  else if (hip_fail(ctx, hipMemsetAsync(A.cells, 0, series_bytes, ctx->stream), "hipMemset(aerosol series)"))  // the series start at 0
    rc = ELMK_E_HIP;
  else
    rc = A.map.upload(ctx, "aerosol", A.mem + A.mem.bytes(), idx, w);
  if (rc != ELMK_OK) A = elmk_ctx::Aerosol{};
  return rc;
}

int elmk_aerosol_upload(elmk_ctx* ctx, int field, int month0, int nmonths, const double* host)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Aerosol& A = ctx->aer;
  if (!A.mem) return invalid(ctx, "elmk_aerosol_upload: elmk_aerosol_reserve has not been called");
  if (!aerosol_field(field)) return invalid(ctx, "elmk_aerosol_upload: not a deposition stream (aer_bcphi .. aer_dst4_2)");
  if (month0 < 0 || nmonths < 1 || month0 + (int64_t)nmonths > RUN_NMONTH) return invalid(ctx, "elmk_aerosol_upload: months outside 0 .. 11");
  if (!host) return invalid(ctx, "elmk_aerosol_upload: null host");
  if (int rc = refuse_capture(ctx, "elmk_aerosol_upload")) return rc;  // (it waits)
  // never write under a reader of these months: the runs that read them, and the stepwise depositions
  if (int rc = wait_for_runs(ctx, [&](int b) { return ((ctx->run.aer_months[b] >> month0) & ((1u << nmonths) - 1u)) != 0; })) return rc;
  if (A.step_live) {
    HIPCHK(hipEventSynchronize(ctx->aer_step_done));
    A.step_live = false;
  }
  const int k = field - ELMK_FIELD_aer_bcphi;
  double* dst = A.cells + ((size_t)k * RUN_NMONTH + (size_t)month0) * (size_t)A.map.ncells;
  HIPCHK(hipMemcpyAsync(dst, host, (size_t)nmonths * (size_t)A.map.ncells * sizeof(double), hipMemcpyHostToDevice, ctx->upload));
  HIPCHK(hipStreamSynchronize(ctx->upload));  // (caller's pageable source; a deposition or run enqueued after this call sees the months)
  return ELMK_OK;
}

int elmk_aerosol_deposition(elmk_ctx* ctx, int month1, int month2, double wt1, double wt2)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Aerosol& A = ctx->aer;
  if (!A.mem) return invalid(ctx, "elmk_aerosol_deposition: elmk_aerosol_reserve has not been called");
  if (month1 < 0 || month1 >= RUN_NMONTH || month2 < 0 || month2 >= RUN_NMONTH) return invalid(ctx, "elmk_aerosol_deposition: month outside 0 .. 11");
  if (!std::isfinite(wt1) || !std::isfinite(wt2)) return invalid(ctx, "elmk_aerosol_deposition: non-finite weight");
  if (int rc = refuse_capture(ctx, "elmk_aerosol_deposition")) return rc;
  if (int rc = heal_lists(ctx)) return rc;
  if (int rc = push_params(ctx)) return rc;
  launch_aerosol_deposition(ctx->d, ctx->ncols, aer_series(ctx), month1, month2, wt1, wt2, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->aer_step_done, ctx->stream));
  A.step_live = true;
  return ELMK_OK;
}

int elmk_aerosol_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_aerosol_clear")) return rc;
  if (int rc = quiesce(ctx, true)) return rc;
  ctx->aer = elmk_ctx::Aerosol{};
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// shortwave: interval-mean FSDS weighted by cos(zenith) (include/elmk.h "shortwave")
// ---------------------------------------------------------------------------------------------------
int elmk_set_shortwave_mode(elmk_ctx* ctx, int mode, double forc_dt_seconds)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Shortwave& W = ctx->sw;
  if (mode != ELMK_SW_REFERENCE && mode != ELMK_SW_COSZEN) return invalid(ctx, "elmk_set_shortwave_mode: unknown mode");
  if (mode == ELMK_SW_COSZEN) {
    if (!ctx->geo_set) return invalid(ctx, "elmk_set_shortwave_mode: COSZEN needs a column geography (elmk_set_column_geography)");
    if (!(forc_dt_seconds > 0.0 && forc_dt_seconds <= 86400.0 * 366.0))
      return invalid(ctx, "elmk_set_shortwave_mode: forc_dt must be finite and in (0, 366 days]");
  }
  if (int rc = refuse_capture(ctx, "elmk_set_shortwave_mode")) return rc;
  if (mode == W.mode && (mode == ELMK_SW_REFERENCE || forc_dt_seconds == W.forc_dt)) return ELMK_OK;  // no change
  if (mode == ELMK_SW_COSZEN && !W.czf) {
    const size_t bytes = (size_t)ctx->ld * sizeof(double);
    if (hip_fail(ctx, W.czf.alloc(bytes), "hipMalloc(shortwave czf)")) return ELMK_E_NOMEM;
    HIPCHK(hipMemsetAsync(W.czf, 0, bytes, ctx->stream));
  }
  return sw_reset(ctx, mode, forc_dt_seconds);
}

int elmk_set_forcing_record_time(elmk_ctx* ctx, double rec_decday)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Shortwave& W = ctx->sw;
  if (W.mode != ELMK_SW_COSZEN) return invalid(ctx, "elmk_set_forcing_record_time: not in shortwave COSZEN mode");
  if (!rec_decday_ok(rec_decday)) return invalid(ctx, "elmk_set_forcing_record_time: bad rec_decday");
  if (int rc = push_params(ctx)) return rc;
  // the record's scalars with the host libm, as elmk_solar_step_consts does for a step (the day-length terms are not read)
  launch_forcing_cosz(ctx->d, ctx->ncols, elmk_solar_step_consts(W.forc_dt, rec_decday, 0), W.czf, ctx->stream);
  HIPCHK(hipGetLastError());
  W.step_time = W.czf_ready = true;
  return ELMK_OK;
}

int elmk_series_record_times(elmk_ctx* ctx, int slot0, int nslots, const double* rec_decday)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Run& R = ctx->run;
  if (!R.mem) return invalid(ctx, "elmk_series_record_times: elmk_run_reserve has not been called");
  if (ctx->sw.mode != ELMK_SW_COSZEN) return invalid(ctx, "elmk_series_record_times: not in shortwave COSZEN mode");
  if (slot0 < 0 || nslots < 0 || slot0 + (int64_t)nslots > R.slots) return invalid(ctx, "elmk_series_record_times: slots out of range");
  if (nslots > 0 && !rec_decday) return invalid(ctx, "elmk_series_record_times: null rec_decday");
  for (int i = 0; i < nslots; i++)
    if (!rec_decday_ok(rec_decday[i])) return invalid(ctx, "elmk_series_record_times: bad rec_decday");
  if (int rc = refuse_capture(ctx, "elmk_series_record_times")) return rc;
  if (nslots == 0) return ELMK_OK;
  if (!R.rec) {
    const size_t bytes = (size_t)R.slots * sizeof(elmk_solar_step);
    if (hip_fail(ctx, R.rec.alloc(bytes), "hipMalloc(record times)")) return ELMK_E_NOMEM;
    R.rec_set.assign((size_t)R.slots, 0);
  }
  // (the runs that read these slots, as elmk_series_upload)
  if (int rc = wait_for_runs(ctx, [&](int b) { return slot0 <= R.slot_hi[b] && slot0 + nslots - 1 >= R.slot_lo[b]; })) return rc;
  std::vector<elmk_solar_step> q((size_t)nslots);
  for (int i = 0; i < nslots; i++) q[(size_t)i] = elmk_solar_step_consts(ctx->sw.forc_dt, rec_decday[i], 0);
  HIPCHK(hipMemcpyAsync(R.rec + slot0, q.data(), q.size() * sizeof(elmk_solar_step), hipMemcpyHostToDevice, ctx->upload));
  HIPCHK(hipStreamSynchronize(ctx->upload));  // (q goes out of scope; a run enqueued after this call sees the times)
  std::fill(R.rec_set.begin() + slot0, R.rec_set.begin() + slot0 + nslots, 1);
  return ELMK_OK;
}

int elmk_download_forcing_cosz(elmk_ctx* ctx, double* czf)
{
  if (int rc = enter(ctx)) return rc;
  if (!czf) return invalid(ctx, "elmk_download_forcing_cosz: null pointer");
  if (!ctx->sw.czf_ready) return invalid(ctx, "elmk_download_forcing_cosz: no record time or COSZEN run step since the mode was set");
  if (int rc = refuse_capture(ctx, "elmk_download_forcing_cosz")) return rc;
  if (ctx->ncols > 0) HIPCHK(hipMemcpyAsync(czf, ctx->sw.czf, (size_t)ctx->ncols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

// ---------------------------------------------------------------------------------------------------
// downscaling: forcing adjusted to each column's elevation (include/elmk.h "downscaling")
// ---------------------------------------------------------------------------------------------------
int elmk_set_column_elevation(elmk_ctx* ctx, const double* topo_col, const double* topo_forc)
{
  if (int rc = enter(ctx)) return rc;
  const int64_t n = ctx->ncols;
  if (!topo_col && n > 0) return invalid(ctx, "elmk_set_column_elevation: null topo_col");
  if (n > 0 && (!all_finite(topo_col, n) || (topo_forc && !all_finite(topo_forc, n))))
    return invalid(ctx, "elmk_set_column_elevation: non-finite elevation");
  if (int rc = refuse_capture(ctx, "elmk_set_column_elevation")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  if (int rc = ds_alloc_topo(ctx)) return rc;
  elmk_ctx::Downscale& D = ctx->ds;
  if (n > 0) {
    HIPCHK(hipMemcpyAsync(D.topo, topo_col, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (topo_forc) HIPCHK(hipMemcpyAsync(D.topo + ctx->ld, topo_forc, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (the caller's pageable arrays)
  D.col_set = true;
  if (topo_forc) D.forc_set = true;
  return ELMK_OK;
}

int elmk_set_forcing_elevation_gridded(elmk_ctx* ctx, const double* cells)
{
  if (int rc = enter(ctx)) return rc;
  const elmk_ctx::Grid& G = ctx->grid;
  if (!G.mem) return invalid(ctx, "elmk_set_forcing_elevation_gridded: no forcing grid (elmk_set_forcing_grid)");
  if (!cells) return invalid(ctx, "elmk_set_forcing_elevation_gridded: null cells");
  if (!all_finite(cells, G.map.ncells)) return invalid(ctx, "elmk_set_forcing_elevation_gridded: non-finite elevation");
  if (int rc = refuse_capture(ctx, "elmk_set_forcing_elevation_gridded")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  if (int rc = ds_alloc_topo(ctx)) return rc;
  elmk_ctx::Downscale& D = ctx->ds;
  if (ctx->ncols > 0) {
    HIPCHK(hipMemcpyAsync(G.cells, cells, (size_t)G.map.ncells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    launch_remap_field_f64(D.topo + ctx->ld, G.cells, ctx->ncols, ctx->ld, G.map.npad, G.map.idx, G.map.w, ctx->stream);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (the staging is reused by the next call)
  D.forc_set = true;
  return ELMK_OK;
}

int elmk_set_downscaling(elmk_ctx* ctx, int mode, double lapse, double lapse_lw, double lw_limit)
{
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Downscale& D = ctx->ds;
  if (mode != ELMK_DS_OFF && mode != ELMK_DS_TOPO) return invalid(ctx, "elmk_set_downscaling: unknown mode");
  if (!(std::isfinite(lapse) && std::isfinite(lapse_lw) && std::isfinite(lw_limit)))
    return invalid(ctx, "elmk_set_downscaling: non-finite parameter");
  if (lapse < 0.0 || lapse_lw < 0.0) return invalid(ctx, "elmk_set_downscaling: negative lapse rate");
  if (!(lw_limit >= 0.0 && lw_limit < 1.0)) return invalid(ctx, "elmk_set_downscaling: lw_limit outside [0, 1)");
  if (mode == ELMK_DS_TOPO && !(D.col_set && D.forc_set))
    return invalid(ctx, "elmk_set_downscaling: TOPO needs both elevations (elmk_set_column_elevation, elmk_set_forcing_elevation_gridded)");
  if (int rc = refuse_capture(ctx, "elmk_set_downscaling")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  D.mode = mode;
  D.lapse = lapse;
  D.lapse_lw = lapse_lw;
  D.lw_limit = lw_limit;
  return ELMK_OK;
}

int elmk_set_downscaling_groups(elmk_ctx* ctx, int64_t ngroups, const int64_t* ptr, const int32_t* col, const double* w)
{
  if (int rc = enter(ctx)) return rc;
  // (every gather and scatter of the renormalisation stays inside the longwave row, and a column is scaled once, because of this check)
  if (int rc = invalid_map(ctx, "elmk_set_downscaling_groups", csr_check(ngroups, ctx->ncols, ptr, col, w, "ngroups outside 1 .. 2^31-1", true, true))) return rc;
  if (int rc = refuse_capture(ctx, "elmk_set_downscaling_groups")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  elmk_ctx::Downscale& D = ctx->ds;
  (void)D.gmem.reset();
  std::vector<double> wsum((size_t)ngroups, 0.0);  // W = w[p0], then W = W + w[p]: the order of agg_cells
  for (int64_t g = 0; g < ngroups; g++)
    for (int64_t p = ptr[g]; p < ptr[g + 1]; p++) wsum[(size_t)g] = p == ptr[g] ? w[p] : wsum[(size_t)g] + w[p];
  int rc = ELMK_OK;
  if (hip_fail(ctx, carve(D.gmem, [&](Carve& L) {
                 D.groups.take(L, ngroups, ptr[ngroups]);
                 L.take(D.wsum, (size_t)ngroups * sizeof(double));
                 L.take(D.lg, (size_t)ctx->ld * sizeof(double));
               }), "hipMalloc(downscaling groups)"))
    rc = ELMK_E_NOMEM;
  else if (hip_fail(ctx, hipMemsetAsync(D.lg, 0, (size_t)ctx->ld * sizeof(double), ctx->stream), "hipMemset(lg)"))
    rc = ELMK_E_HIP;
  else
    rc = D.groups.upload(ctx, ptr, col, w, [&] {
      return hip_fail(ctx, hipMemcpyAsync(D.wsum, wsum.data(), (size_t)ngroups * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(wsum)");
    });
  if (rc != ELMK_OK) {
    (void)D.gmem.reset();
    D.groups = CsrMap{};
  }
  return rc;
}

int elmk_clear_downscaling_groups(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_clear_downscaling_groups")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  elmk_ctx::Downscale& D = ctx->ds;
  D.groups = CsrMap{};
  HIPCHK(D.gmem.reset());
  return ELMK_OK;
}

int elmk_download_column_elevation(elmk_ctx* ctx, double* topo_col, double* topo_forc)
{
  if (int rc = enter(ctx)) return rc;
  const elmk_ctx::Downscale& D = ctx->ds;
  if ((topo_col && !D.col_set) || (topo_forc && !D.forc_set)) return invalid(ctx, "elmk_download_column_elevation: not set");
  if (int rc = refuse_capture(ctx, "elmk_download_column_elevation")) return rc;
  const size_t bytes = (size_t)ctx->ncols * sizeof(double);
  if (topo_col && bytes) HIPCHK(hipMemcpyAsync(topo_col, D.topo, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (topo_forc && bytes) HIPCHK(hipMemcpyAsync(topo_forc, D.topo + ctx->ld, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

}  // extern "C"
