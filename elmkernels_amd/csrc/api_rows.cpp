// api_rows.cpp - the features that keep fp64 rows [row][ld] of their own beside the state, held exactly while the feature is enabled:
// active layer thickness (k_active_layer.hip), soil hydrology and its frost-table extension (k_soil_hydrology.hip), the water balance
// (k_water_balance.hip); include/elmk.h under those names.  The irrigation's rows are api_irrigation.cpp's.
#include "elmk_ctx.h"

namespace {
static_assert(ELMK_ALT_ALT == 0 && ELMK_ALT_ALTMAX_LASTYEAR == ALT_NROWS - 1, "three rows");
constexpr Rows ALT{&elmk_ctx::alt_rows, ALT_NROWS, "active layer", "elmk_active_layer_enable", ELMK_ROWS_ALT};
constexpr Rows HYD{&elmk_ctx::hyd_rows, ELMK_HYD_NROWS, "soil hydrology", "elmk_soil_hydrology_enable", ELMK_ROWS_HYDROLOGY};
constexpr Rows HYDF{&elmk_ctx::hydf_rows, ELMK_HYDF_NROWS, "frost table", "elmk_soil_hydrology_frost_enable", ELMK_ROWS_FROST};
constexpr Rows WB{&elmk_ctx::wb_rows, ELMK_WB_NROWS, "water balance", "elmk_water_balance_enable", ELMK_ROWS_WATER_BALANCE};
const Rows* const FAMILY[ELMK_ROWS_NFAMILY] = {&ALT, &HYD, &HYDF, &WB, &ROWS_OF_IRRIGATION};
}  // namespace

namespace elmk {
// while a history entry reads the family's rows they stay: "<who>: history entries over the rows exist (elmk_history_clear first)"
int rows_held(elmk_ctx* ctx, const Rows& R, const char* who)
{
  if (!hist_has_family(ctx, R.family)) return points_hold_family(ctx, who, R.family);
  return invalid(ctx, (std::string(who) + ": history entries over the " + R.label + " rows exist (elmk_history_clear first)").c_str());
}

// how every call but enable and clear begins
int rows_enter(elmk_ctx* ctx, const Rows& R, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  return ctx->*R.buf ? ELMK_OK : invalid(ctx, (std::string(who) + ": not enabled (" + R.enable + ")").c_str());
}

// columns [col0, col0 + n) of one row; synchronises
int rows_read(elmk_ctx* ctx, const Rows& R, const char* who, int which, double* host, int64_t col0, int64_t n)
{
  if (int rc = rows_enter(ctx, R, who)) return rc;
  if (which < 0 || which >= R.nrows) return invalid(ctx, (std::string(who) + ": unknown row").c_str());
  if (int rc = check_range(ctx, who, host, col0, n, ctx->ncols)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  const double* rows = ctx->*R.buf;
  if (n > 0) HIPCHK(hipMemcpyAsync(host, rows + (size_t)which * (size_t)ctx->ld + (size_t)col0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int rows_clear(elmk_ctx* ctx, const Rows& R, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (!(ctx->*R.buf)) return ELMK_OK;
  if (int rc = rows_held(ctx, R, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  HIPCHK((ctx->*R.buf).reset());
  return ELMK_OK;
}

}  // namespace elmk

namespace {
// allocate and zero the rows; nothing is held after a failure
int rows_enable(elmk_ctx* ctx, const Rows& R, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  DevBuf<double>& buf = ctx->*R.buf;
  if (buf) return invalid(ctx, (std::string(who) + ": already enabled").c_str());
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its flags' moment)
  const size_t bytes = (size_t)R.nrows * (size_t)ctx->ld * sizeof(double);
  const std::string what = std::string("(") + R.label + " rows)";
  if (hip_fail(ctx, buf.alloc(bytes), ("hipMalloc" + what).c_str())) return ELMK_E_NOMEM;
  if (hip_fail(ctx, hipMemsetAsync(buf, 0, bytes, ctx->stream), ("hipMemset" + what).c_str()) ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)buf.reset();
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

// the water balance's scratch and ring rows go with its rows
void wb_release(elmk_ctx* ctx)
{
  (void)ctx->wb_rows.reset();
  (void)ctx->wb_red.reset();
  (void)ctx->wb_ring.reset();
  ctx->wb_part = ctx->wb_out = ctx->wb_ring_mms = nullptr;
  ctx->wb_census = ctx->wb_ring_census = nullptr;
  ctx->wb_ran = ctx->wb_ran_empty = false;
}

// what zero columns reduce to
void wb_identity(double* mms, int64_t* nbad, int64_t* first)
{
  for (int k = 0; mms && k < 3; k++) {
    mms[3 * k] = INFINITY;
    mms[3 * k + 1] = -INFINITY;
    mms[3 * k + 2] = 0.0;
  }
  if (nbad) *nbad = 0;
  if (first) *first = -1;
}
constexpr long long WB_NONE = 0x7fffffffffffffffll;
}  // namespace

namespace elmk {
ActiveLayerArgs alt_args(const elmk_ctx* ctx)
{
  return ActiveLayerArgs{ctx->fptr[ELMK_FIELD_t_soisno], ctx->fptr[ELMK_FIELD_zsoi], (int32_t*)ctx->fptr[ELMK_FIELD_altmax_indx],
                         (int32_t*)ctx->fptr[ELMK_FIELD_altmax_lastyear_indx], ctx->alt_rows,
                         ctx->geo + (size_t)ELMK_GEO_SIN_LAT * (size_t)ctx->ld, ctx->ld, ctx->ncols};
}
bool hyd_land(const elmk_ctx* ctx) { return ctx->h.land.ltype == istsoil || ctx->h.land.ltype == istcrop; }
void hyd_launch(elmk_ctx* ctx, double dt)
{
  if (!hyd_land(ctx)) return;
  const elmk_ctx::Routing& T = ctx->route;
  if (ctx->hs.mem) {  // L1 and L2, then the LAT form, exactly while the hillslope lateral flow is on (it excludes the two forms below)
    const elmk_ctx::Hillslope& H = ctx->hs;
    launch_hillslope(ctx->d, ctx->ncols, ctx->ld, ctx->hyd_rows, HillslopeArgs{H.rows, H.geom, H.down, H.up, H.npad, H.k_aniso}, ctx->stream);
    const LatArgs lat{H.rows + (size_t)ELMK_HS_QLAT_NET * (size_t)ctx->ld, H.down};
    launch_soil_hydrology(ctx->d, ctx->ncols, ctx->hyd_rows, nullptr, dt, ctx->stream, nullptr, &lat);
    return;
  }
  if (T.land.mem) {  // the ROF form exactly while the floodplain infiltration is on
    const size_t cld = (size_t)T.cld;
    const RofArgs rof{T.land_cellof, T.fp.rows + FP_WF * cld, T.fp.rows + FP_FRAC * cld, T.area, T.land.tab};
    launch_soil_hydrology(ctx->d, ctx->ncols, ctx->hyd_rows, ctx->hydf_rows, dt, ctx->stream, &rof);
  } else {
    launch_soil_hydrology(ctx->d, ctx->ncols, ctx->hyd_rows, ctx->hydf_rows, dt, ctx->stream);
  }
}
void wb_begin_launch(elmk_ctx* ctx)
{
  if (hyd_land(ctx)) launch_wb_begin(ctx->d, ctx->ncols, ctx->hyd_rows, ctx->wb_rows, ctx->stream);
}
// run: the triples and the census into the ring rows of the step the device cursor names
void wb_launch(elmk_ctx* ctx, double dt, bool run)
{
  if (!hyd_land(ctx)) return;
  launch_water_balance(ctx->d, ctx->ncols, ctx->ld, ctx->hyd_rows, ctx->hydf_rows, ctx->wb_rows, dt, ctx->wb_tol, ctx->wb_part, ctx->wb_out,
                       run ? ctx->wb_ring_mms : nullptr, run ? ctx->wb_ring_census : ctx->wb_census, run ? ctx->run.cursor : nullptr,
                       ctx->stream, ctx->irr_rows ? ctx->irr_rows + (size_t)ELMK_IRR_QFLX_IRRIG * (size_t)ctx->ld : nullptr,
                       ctx->route.land.mem ? ctx->route.land.tab + (size_t)ELMK_FPI_QFLX_DRAIN * (size_t)ctx->ld : nullptr);
}
int wb_ring_alloc(elmk_ctx* ctx)
{
  (void)ctx->wb_ring.reset();
  ctx->wb_ring_mms = nullptr;
  ctx->wb_ring_census = nullptr;
  if (!ctx->wb_rows || !ctx->run.mem) return ELMK_OK;
  const size_t nrow = 2 * (size_t)ctx->run.max_steps;
  if (hip_fail(ctx, carve(ctx->wb_ring, [&](Carve& L) {
                 L.take(ctx->wb_ring_mms, nrow * 9 * sizeof(double));
                 L.take(ctx->wb_ring_census, nrow * 2 * sizeof(long long));
               }), "hipMalloc(water balance ring)"))
    return ELMK_E_NOMEM;
  if (hip_fail(ctx, hipMemsetAsync(ctx->wb_ring, 0, ctx->wb_ring.bytes(), ctx->stream), "hipMemset(water balance ring)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->wb_ring.reset();
    ctx->wb_ring_mms = nullptr;
    ctx->wb_ring_census = nullptr;
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}
const double* feature_row(const elmk_ctx* ctx, int family, int which, const char** why)
{
  if (family == ELMK_ROWS_FLOODPLAIN) {  // (the extension's column rows lie in the river stage's allocation)
    if (!ctx->route.land.mem) return *why = "the family's feature is not enabled", nullptr;
    if (which < 0 || which >= ELMK_FPI_NROWS) return *why = "unknown row", nullptr;
    return ctx->route.land.tab + (size_t)which * (size_t)ctx->ld;
  }
  if (family == ELMK_ROWS_HILLSLOPE) {  // (the extension's rows lie in its own allocation)
    if (!ctx->hs.mem) return *why = "the family's feature is not enabled", nullptr;
    if (which < 0 || which >= ELMK_HS_NROWS) return *why = "unknown row", nullptr;
    return ctx->hs.rows + (size_t)which * (size_t)ctx->ld;
  }
  if (family < 0 || family >= ELMK_ROWS_NFAMILY) return *why = "unknown row family", nullptr;
  const Rows& R = *FAMILY[family];
  if (!(ctx->*R.buf)) return *why = "the family's feature is not enabled", nullptr;
  if (which < 0 || which >= R.nrows) return *why = "unknown row", nullptr;
  return (const double*)(ctx->*R.buf) + (size_t)which * (size_t)ctx->ld;
}
}  // namespace elmk

extern "C" {

// ---------------------------------------------------------------------------------------------------
// active layer thickness
// ---------------------------------------------------------------------------------------------------
int elmk_active_layer_enable(elmk_ctx* ctx) { return rows_enable(ctx, ALT, "elmk_active_layer_enable"); }

int elmk_active_layer_init(elmk_ctx* ctx, const double* altmax, const double* altmax_lastyear)
{
  if (int rc = rows_enter(ctx, ALT, "elmk_active_layer_init")) return rc;
  if (int rc = refuse_capture(ctx, "elmk_active_layer_init")) return rc;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  HIPCHK(hipMemsetAsync(ctx->alt_rows, 0, ctx->alt_rows.bytes(), ctx->stream));
  if (altmax && n) HIPCHK(hipMemcpyAsync(ctx->alt_rows + ELMK_ALT_ALTMAX * ld, altmax, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (altmax_lastyear && n)
    HIPCHK(hipMemcpyAsync(ctx->alt_rows + ELMK_ALT_ALTMAX_LASTYEAR * ld, altmax_lastyear, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_active_layer_update(elmk_ctx* ctx, int rollover)
{
  if (int rc = rows_enter(ctx, ALT, "elmk_active_layer_update")) return rc;
  if (!ctx->geo_set) return invalid(ctx, "elmk_active_layer_update: no column geography (elmk_set_column_geography)");
  if (rollover & ~(ELMK_ALT_ROLL_NORTH | ELMK_ALT_ROLL_SOUTH)) return invalid(ctx, "elmk_active_layer_update: unknown rollover bits");
  launch_active_layer(alt_args(ctx), rollover, ctx->stream);
  return launched(ctx);
}

int elmk_active_layer_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, ALT, "elmk_active_layer_read", w, host, col0, n); }

int elmk_active_layer_clear(elmk_ctx* ctx) { return rows_clear(ctx, ALT, "elmk_active_layer_clear"); }

// ---------------------------------------------------------------------------------------------------
// soil hydrology
// ---------------------------------------------------------------------------------------------------
int elmk_soil_hydrology_enable(elmk_ctx* ctx)
{
  const int rc = rows_enable(ctx, HYD, "elmk_soil_hydrology_enable");
  if (rc == ELMK_OK) ctx->hyd_params = false;
  return rc;
}

int elmk_soil_hydrology_set_params(elmk_ctx* ctx, const double* hksat, const double* wtfact, const double* h2osfc_thresh,
                                   const double* k_wet, const double* rsub_top_max)
{
  if (int rc = rows_enter(ctx, HYD, "elmk_soil_hydrology_set_params")) return rc;
  if (!hksat || !wtfact || !h2osfc_thresh || !k_wet || !rsub_top_max) return invalid(ctx, "elmk_soil_hydrology_set_params: null argument");
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_set_params")) return rc;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  if (n) {
    HIPCHK(hipMemcpy2DAsync(ctx->hyd_rows + ELMK_HYD_HKSAT * ld, ld * 8, hksat, n * 8, n * 8, ELMK_HYD_NLAYER, hipMemcpyHostToDevice,
                            ctx->stream));
    const double* one[4] = {wtfact, h2osfc_thresh, k_wet, rsub_top_max};
    for (int k = 0; k < 4; k++)
      HIPCHK(hipMemcpyAsync(ctx->hyd_rows + (size_t)(ELMK_HYD_WTFACT + k) * ld, one[k], n * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->hyd_params = true;
  return ELMK_OK;
}

int elmk_soil_hydrology_init(elmk_ctx* ctx, const double* zwt, const double* wa)
{
  if (int rc = rows_enter(ctx, HYD, "elmk_soil_hydrology_init")) return rc;
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_init")) return rc;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  std::vector<double> cold;
  if (n && (!zwt || !wa)) {
    // ELM's cold start: wa = 4000 mm, zwt = (zi[9] + 25) - wa / 0.2 / 1000 from the bottom of layer 9 (level 15 of zisoi, as stored)
    cold.assign(n, 4000.0);
    if (!zwt) {
      const int es = store_size(ELMK_F64);
      std::vector<unsigned char> raw(n * (size_t)es);
      HIPCHK(hipMemcpyAsync(raw.data(), (const char*)ctx->fptr[ELMK_FIELD_zisoi] + (size_t)(ELMK_NLEVSNO + ELMK_HYD_NLAYER) * ld * es,
                            raw.size(), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));
      std::vector<double> z(n);
      for (size_t i = 0; i < n; i++) {
        double zi9;
        if (es == 4) {
          float f;
          memcpy(&f, &raw[i * 4], 4);
          zi9 = (double)f;
        } else {
          memcpy(&zi9, &raw[i * 8], 8);
        }
        z[i] = (zi9 + 25.0) - 4000.0 / 0.2 / 1000.0;
      }
      HIPCHK(hipMemcpyAsync(ctx->hyd_rows + ELMK_HYD_ZWT * ld, z.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(hipStreamSynchronize(ctx->stream));  // (z leaves scope)
    }
  }
  if (n && zwt) HIPCHK(hipMemcpyAsync(ctx->hyd_rows + ELMK_HYD_ZWT * ld, zwt, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (n) HIPCHK(hipMemcpyAsync(ctx->hyd_rows + ELMK_HYD_WA * ld, wa ? wa : cold.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_soil_hydrology(elmk_ctx* ctx, double dt)
{
  if (int rc = rows_enter(ctx, HYD, "elmk_soil_hydrology")) return rc;
  if (!ctx->hyd_params) return invalid(ctx, "elmk_soil_hydrology: the parameters are not set (elmk_soil_hydrology_set_params)");
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_soil_hydrology: dt must be finite and positive");
  if (int rc = enter_physics(ctx)) return rc;
  hyd_launch(ctx, dt);
  return launched(ctx);
}

int elmk_soil_hydrology_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, HYD, "elmk_soil_hydrology_read", w, host, col0, n); }

int elmk_soil_hydrology_clear(elmk_ctx* ctx)
{
  const char* who = "elmk_soil_hydrology_clear";
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  for (const Rows* R : {&HYD, &HYDF, &WB})  // nothing changes unless all three may go
    if (int rc = rows_held(ctx, *R, who)) return rc;
  if (int rc = land_holds(ctx, who)) return rc;  // (the hydrology's ROF form and the water balance's LAND form go with their rows)
  if (int rc = route_holds(ctx, who)) return rc;  // (the routing reads the water balance's QRUNOFF)
  if (int rc = hs_held(ctx, who)) return rc;
  if (int rc = elmk_water_balance_clear(ctx)) return rc;
  if (int rc = rows_clear(ctx, HYDF, who)) return rc;
  if (ctx->hs.mem) {  // the hillslope lateral flow goes with the stage it extends
    if (int rc = quiesce(ctx, false)) return rc;
    hs_release(ctx);
  }
  const int rc = rows_clear(ctx, HYD, who);
  if (rc == ELMK_OK) ctx->hyd_params = false;
  return rc;
}

// the frost-table extension: rows of its own beside the hydrology's, so that ELMK_HYD_NROWS stays what it is
int elmk_soil_hydrology_frost_enable(elmk_ctx* ctx, const double* q_perch_max)
{
  const char* who = "elmk_soil_hydrology_frost_enable";
  if (int rc = rows_enter(ctx, HYD, who)) return rc;
  if (!q_perch_max) return invalid(ctx, "elmk_soil_hydrology_frost_enable: null argument");
  if (int rc = hs_excludes(ctx, who)) return rc;  // (F'.A skips F.1 and F.2, which would drop a flux the neighbours have booked)
  if (int rc = rows_held(ctx, HYDF, who)) return rc;  // (a second enable: refused under row entries as the clear is)
  if (int rc = rows_enable(ctx, HYDF, who)) return rc;  // (zero-filled: the diagnostics)
  const size_t n = (size_t)ctx->ncols;
  if (n && (hip_fail(ctx, hipMemcpyAsync(ctx->hydf_rows + (size_t)ELMK_HYDF_Q_PERCH_MAX * (size_t)ctx->ld, q_perch_max, n * 8, hipMemcpyHostToDevice, ctx->stream),
                     "hipMemcpy(frost table rows)") ||
            hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->hydf_rows.reset();
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

int elmk_soil_hydrology_frost_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, HYDF, "elmk_soil_hydrology_frost_read", w, host, col0, n); }

int elmk_soil_hydrology_frost_clear(elmk_ctx* ctx) { return rows_clear(ctx, HYDF, "elmk_soil_hydrology_frost_clear"); }

// ---------------------------------------------------------------------------------------------------
// water balance
// ---------------------------------------------------------------------------------------------------
int elmk_water_balance_enable(elmk_ctx* ctx, double tol_mm)
{
  const char* who = "elmk_water_balance_enable";
  if (int rc = rows_enter(ctx, HYD, who)) return rc;
  if (!(std::isfinite(tol_mm) && tol_mm >= 0.0)) return invalid(ctx, "elmk_water_balance_enable: tol_mm must be finite and not negative");
  if (int rc = rows_enable(ctx, WB, who)) return rc;
  int rc = hip_fail(ctx, carve(ctx->wb_red, [&](Carve& L) {
                      L.take(ctx->wb_part, (size_t)3 * ELMK_CONS_NPART * 3 * sizeof(double));
                      L.take(ctx->wb_out, 256);  // the triples, and the census behind them
                    }), "hipMalloc(water balance reduction)")
               ? ELMK_E_NOMEM
               : ELMK_OK;
  if (rc == ELMK_OK) {
    ctx->wb_census = (long long*)(ctx->wb_out + 16);
    rc = wb_ring_alloc(ctx);
  }
  if (rc != ELMK_OK) {
    wb_release(ctx);
    return rc;
  }
  ctx->wb_tol = tol_mm;
  return ELMK_OK;
}

int elmk_water_balance_begin(elmk_ctx* ctx)
{
  if (int rc = rows_enter(ctx, WB, "elmk_water_balance_begin")) return rc;
  if (int rc = enter_physics(ctx)) return rc;
  wb_begin_launch(ctx);
  return launched(ctx);
}

int elmk_water_balance(elmk_ctx* ctx, double dt, double* min_max_sum, int64_t* nbad, int64_t* first_bad_col)
{
  if (int rc = rows_enter(ctx, WB, "elmk_water_balance")) return rc;
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_water_balance: dt must be finite and positive");
  const bool reads = min_max_sum || nbad || first_bad_col;
  if (reads)
    if (int rc = refuse_capture(ctx, "elmk_water_balance")) return rc;
  if (int rc = enter_physics(ctx)) return rc;
  wb_launch(ctx, dt, false);
  if (!reads) return launched(ctx);
  HIPCHK(hipGetLastError());
  if (!hyd_land(ctx) || ctx->ncols <= 0) {
    wb_identity(min_max_sum, nbad, first_bad_col);
    return synced(ctx);
  }
  long long cen[2] = {0, WB_NONE};
  if (min_max_sum) HIPCHK(hipMemcpyAsync(min_max_sum, ctx->wb_out, 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cen, ctx->wb_census, sizeof cen, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (nbad) *nbad = (int64_t)cen[0];
  if (first_bad_col) *first_bad_col = cen[1] == WB_NONE ? -1 : (int64_t)cen[1];
  return ELMK_OK;
}

int elmk_water_balance_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, WB, "elmk_water_balance_read", w, host, col0, n); }

int elmk_water_balance_clear(elmk_ctx* ctx)
{
  if (ctx && ctx->wb_rows) {
    if (int rc = land_holds(ctx, "elmk_water_balance_clear")) return rc;
    if (int rc = route_holds(ctx, "elmk_water_balance_clear")) return rc;
  }
  if (int rc = rows_clear(ctx, WB, "elmk_water_balance_clear")) return rc;
  if (!ctx->wb_rows) wb_release(ctx);  // (rows_clear has made the stream idle)
  return ELMK_OK;
}

int elmk_run_water_balance(elmk_ctx* ctx, double* min_max_sum, int64_t* nbad, int64_t* first_bad_col)
{
  if (int rc = enter(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  const elmk_ctx::Run& R = ctx->run;
  if (R.last_buf < 0 || !ctx->wb_ran) return 0;
  const size_t row0 = (size_t)R.last_buf * R.max_steps, n = (size_t)R.last_nsteps;
  if (ctx->wb_ran_empty) {
    for (size_t i = 0; i < n; i++) wb_identity(min_max_sum ? min_max_sum + 9 * i : nullptr, nbad ? nbad + i : nullptr, first_bad_col ? first_bad_col + i : nullptr);
    return (int)n;
  }
  std::vector<long long> cen(2 * n);
  if (min_max_sum) HIPCHK(hipMemcpyAsync(min_max_sum, ctx->wb_ring_mms + row0 * 9, n * 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(cen.data(), ctx->wb_ring_census + row0 * 2, n * 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++) {
    if (nbad) nbad[i] = (int64_t)cen[2 * i];
    if (first_bad_col) first_bad_col[i] = cen[2 * i + 1] == WB_NONE ? -1 : (int64_t)cen[2 * i + 1];
  }
  return (int)n;
}

}  // extern "C"
