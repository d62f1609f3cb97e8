// api_irrigation.cpp - irrigation (k_irrigation.hip; include/elmk.h "irrigation"): the three fp64 rows RATE, NLEFT, QFLX_IRRIG and the
// int32 parameter row sched, in one allocation held exactly while the feature is enabled.
#include "elmk_ctx.h"

namespace elmk {
static_assert(ELMK_IRR_RATE == 0 && ELMK_IRR_QFLX_IRRIG == IRR_NROWS - 1, "three rows");
const Rows ROWS_OF_IRRIGATION{&elmk_ctx::irr_rows, IRR_NROWS, "irrigation", "elmk_irrigation_enable", ELMK_ROWS_IRRIGATION};

void irr_run_launch(elmk_ctx* ctx, double dt)
{
  if (hyd_land(ctx))
    launch_irrigation_run(ctx->d, ctx->ncols, ctx->irr_rows, ctx->irr_sched, (int)dt, ctx->run.table, ctx->run.cursor, ctx->stream);
}
}  // namespace elmk

namespace {
constexpr const Rows& IRR = ROWS_OF_IRRIGATION;
}

extern "C" {

int elmk_irrigation_enable(elmk_ctx* ctx, const int32_t* sched)
{
  const char* who = "elmk_irrigation_enable";
  if (int rc = enter(ctx)) return rc;
  if (ctx->irr_rows) return invalid(ctx, "elmk_irrigation_enable: already enabled");
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  if (!sched && n > 0) return invalid(ctx, "elmk_irrigation_enable: null argument");
  for (size_t i = 0; i < n; i++)
    if (sched[i] < -1 || sched[i] > 86399) return invalid(ctx, "elmk_irrigation_enable: sched outside -1 .. 86399");
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its flags' moment)
  const size_t row_bytes = (size_t)IRR_NROWS * ld * sizeof(double), bytes = row_bytes + ld * sizeof(int32_t);
  if (hip_fail(ctx, ctx->irr_rows.alloc(bytes), "hipMalloc(irrigation rows)")) return ELMK_E_NOMEM;
  ctx->irr_sched = (int32_t*)((char*)(double*)ctx->irr_rows + row_bytes);
  // the rows zero; sched -1 in the padding columns, then the caller's values
  if (hip_fail(ctx, hipMemsetAsync(ctx->irr_rows, 0, row_bytes, ctx->stream), "hipMemset(irrigation rows)") ||
      hip_fail(ctx, hipMemsetAsync(ctx->irr_sched, 0xFF, ld * sizeof(int32_t), ctx->stream), "hipMemset(irrigation sched)") ||
      (n > 0 && hip_fail(ctx, hipMemcpyAsync(ctx->irr_sched, sched, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream),
                         "hipMemcpy(irrigation sched)")) ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->irr_rows.reset();
    ctx->irr_sched = nullptr;
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

int elmk_irrigation_init(elmk_ctx* ctx, const double* rate, const double* nleft)
{
  const char* who = "elmk_irrigation_init";
  if (int rc = rows_enter(ctx, IRR, who)) return rc;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  for (size_t i = 0; rate && i < n; i++)
    if (!(std::isfinite(rate[i]) && rate[i] >= 0.0)) return invalid(ctx, "elmk_irrigation_init: rate must be finite and not negative");
  for (size_t i = 0; nleft && i < n; i++)
    if (!(nleft[i] >= 0.0 && nleft[i] <= 86400.0 && nleft[i] == std::floor(nleft[i])))
      return invalid(ctx, "elmk_irrigation_init: nleft must be a whole number in 0 .. 86400");
  if (int rc = refuse_capture(ctx, who)) return rc;
  HIPCHK(hipMemsetAsync(ctx->irr_rows, 0, (size_t)IRR_NROWS * ld * sizeof(double), ctx->stream));
  if (rate && n) HIPCHK(hipMemcpyAsync(ctx->irr_rows + ELMK_IRR_RATE * ld, rate, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (nleft && n) HIPCHK(hipMemcpyAsync(ctx->irr_rows + ELMK_IRR_NLEFT * ld, nleft, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_irrigation(elmk_ctx* ctx, double dt, int tod_seconds)
{
  if (int rc = rows_enter(ctx, IRR, "elmk_irrigation")) return rc;
  if (!(dt >= 1.0 && dt <= 86400.0 && dt == std::floor(dt)))
    return invalid(ctx, "elmk_irrigation: dt must be a whole number of seconds in 1 .. 86400");
  if (tod_seconds < 0 || tod_seconds > 86399) return invalid(ctx, "elmk_irrigation: tod_seconds outside 0 .. 86399");
  if (int rc = enter_physics(ctx)) return rc;
  if (hyd_land(ctx)) launch_irrigation(ctx->d, ctx->ncols, ctx->irr_rows, ctx->irr_sched, (int)dt, tod_seconds, ctx->stream);
  return launched(ctx);
}

int elmk_irrigation_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, IRR, "elmk_irrigation_read", w, host, col0, n); }

int elmk_irrigation_clear(elmk_ctx* ctx)
{
  if (ctx && ctx->irr_rows)
    if (int rc = route_holds(ctx, "elmk_irrigation_clear", true)) return rc;  // (the withdrawal reads QFLX_IRRIG)
  const int rc = rows_clear(ctx, IRR, "elmk_irrigation_clear");
  if (rc == ELMK_OK && !ctx->irr_rows) ctx->irr_sched = nullptr;
  return rc;
}

}  // extern "C"
