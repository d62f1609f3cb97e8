// api_hillslope.cpp - the hillslope lateral flow (elmk_hillslope_*; include/elmk.h "hillslope lateral flow"): an extension of the soil
// hydrology stage with one allocation of its own, held exactly while it is on.  The checks and the uphill map are elmk_maps.h:
// hillslope_check's; the launches are api_rows.cpp: hyd_launch's (k_hillslope.hip, then k_soil_hydrology.hip's LAT form).
#include "elmk_ctx.h"

namespace elmk {
int hs_excludes(elmk_ctx* ctx, const char* who)
{
  return ctx->hs.mem ? invalid(ctx, (std::string(who) + ": the hillslope lateral flow is on (elmk_hillslope_clear first)").c_str()) : ELMK_OK;
}

int hs_held(elmk_ctx* ctx, const char* who)
{
  if (!ctx->hs.mem) return ELMK_OK;
  if (hist_has_family(ctx, ELMK_ROWS_HILLSLOPE))
    return invalid(ctx, (std::string(who) + ": history entries over the hillslope rows exist (elmk_history_clear first)").c_str());
  return points_hold_family(ctx, who, ELMK_ROWS_HILLSLOPE);
}

void hs_release(elmk_ctx* ctx)
{
  (void)ctx->hs.mem.reset();
  ctx->hs = elmk_ctx::Hillslope{};
}
}  // namespace elmk

namespace {
int hs_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  return ctx->hs.mem ? ELMK_OK : invalid(ctx, (std::string(who) + ": not enabled (elmk_hillslope_enable)").c_str());
}
}  // namespace

extern "C" {

int elmk_hillslope_enable(elmk_ctx* ctx, const int32_t* down, const double* dist, const double* width, const double* area, const double* elev,
                          double k_aniso)
{
  const char* who = "elmk_hillslope_enable";
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_hillslope_enable: the soil hydrology is not enabled (elmk_soil_hydrology_enable)");
  elmk_ctx::Hillslope& H = ctx->hs;
  if (H.mem) return invalid(ctx, "elmk_hillslope_enable: already on");
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (!down || !dist || !width || !area || !elev) return invalid(ctx, "elmk_hillslope_enable: null argument");
  if (ctx->hydf_rows) return invalid(ctx, "elmk_hillslope_enable: the frost table is on (elmk_soil_hydrology_frost_clear first)");
  if (ctx->route.land.mem) return invalid(ctx, "elmk_hillslope_enable: the floodplain infiltration is on (elmk_floodplain_infiltration_clear first)");
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  int nup = 0;
  int64_t col = -1;
  std::vector<int32_t> up;
  if (const char* text = hillslope_check(ctx->ncols, down, dist, width, area, elev, k_aniso, ctx->ld, &nup, &up, &col))
    return invalid(ctx, (std::string(who) + ": " + text + (col >= 0 ? " at column " + std::to_string(col) : std::string())).c_str());
  const int npad = ell_npad(nup);
  if (hip_fail(ctx, carve(H.mem, [&](Carve& L) {
                 L.take(H.rows, (size_t)ELMK_HS_NROWS * ld * sizeof(double));
                 L.take(H.geom, (size_t)HS_NGEOM * ld * sizeof(double));
                 L.take(H.down, ld * sizeof(int32_t));
                 L.take(H.up, (size_t)npad * ld * sizeof(int32_t));
                 L.take(H.part, (size_t)ELMK_CONS_NPART * 3 * sizeof(double));
                 L.take(H.out, 256);
               }), "hipMalloc(hillslope)")) {
    hs_release(ctx);
    return ELMK_E_NOMEM;
  }
  // The captured run step holds the stage of its moment: dropped once the memory is there.  If a copy below fails the extension is off
  // again and the step stays dropped; the next run captures it anew.
  if (int rc = quiesce(ctx, false)) {
    hs_release(ctx);
    return rc;
  }
  // the rows zero; the geometry's padding columns 1.0 (nothing divides by a zero there) under down -2; then the caller's arrays
  std::vector<double> geom((size_t)HS_NGEOM * ld, 1.0);
  std::vector<int32_t> dn(ld, -2);
  const double* const src[HS_NGEOM] = {dist, width, area, elev};
  for (int k = 0; k < HS_NGEOM; k++) std::copy(src[k], src[k] + n, geom.begin() + (size_t)k * ld);
  std::copy(down, down + n, dn.begin());
  if (hip_fail(ctx, hipMemsetAsync(H.mem, 0, H.mem.bytes(), ctx->stream), "hipMemset(hillslope)") ||
      hip_fail(ctx, hipMemcpyAsync(H.geom, geom.data(), geom.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(hillslope geometry)") ||
      hip_fail(ctx, hipMemcpyAsync(H.down, dn.data(), dn.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(hillslope down)") ||
      hip_fail(ctx, hipMemcpyAsync(H.up, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(hillslope map)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    hs_release(ctx);
    return ELMK_E_HIP;
  }
  H.npad = npad;
  H.k_aniso = k_aniso;
  return ELMK_OK;
}

int elmk_hillslope_read(elmk_ctx* ctx, int which, double* host, int64_t col0, int64_t n)
{
  const char* who = "elmk_hillslope_read";
  if (int rc = hs_enter(ctx, who)) return rc;
  if (which < 0 || which >= ELMK_HS_NROWS) return invalid(ctx, "elmk_hillslope_read: unknown row");
  if (int rc = check_range(ctx, who, host, col0, n, ctx->ncols)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (n > 0) HIPCHK(hipMemcpyAsync(host, ctx->hs.rows + (size_t)which * (size_t)ctx->ld + (size_t)col0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int elmk_hillslope_budget(elmk_ctx* ctx, double* sums)
{
  const char* who = "elmk_hillslope_budget";
  if (int rc = hs_enter(ctx, who)) return rc;
  if (!sums) return invalid(ctx, "elmk_hillslope_budget: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const elmk_ctx::Hillslope& H = ctx->hs;
  double mms[3] = {INFINITY, -INFINITY, 0.0};
  if (ctx->ncols > 0) {
    launch_min_max_sum(H.rows + (size_t)ELMK_HS_QSTREAM * (size_t)ctx->ld, ctx->ld, ctx->ncols, 1, H.part, H.out, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mms, H.out, sizeof mms, hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  sums[0] = mms[2];
  return ELMK_OK;
}

int elmk_hillslope_clear(elmk_ctx* ctx)
{
  const char* who = "elmk_hillslope_clear";
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (!ctx->hs.mem) return ELMK_OK;
  if (int rc = hs_held(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  hs_release(ctx);
  return ELMK_OK;
}

}  // extern "C"
