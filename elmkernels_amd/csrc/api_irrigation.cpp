// api_irrigation.cpp - irrigation (k_irrigation.hip; include/elmk.h "irrigation"): the three fp64 rows RATE, NLEFT, QFLX_IRRIG and the
// int32 parameter row sched, in one allocation held exactly while the feature is enabled; and its river supply limit
// (k_irrigation_supply in k_history.hip; include/elmk.h "irrigation: river supply limit"): four fp64 cell rows held exactly while the
// limit is on.
#include "elmk_ctx.h"

namespace elmk {
static_assert(ELMK_IRR_RATE == 0 && ELMK_IRR_QFLX_IRRIG == IRR_NROWS - 1, "three rows");
const Rows ROWS_OF_IRRIGATION{&elmk_ctx::irr_rows, IRR_NROWS, "irrigation", "elmk_irrigation_enable", ELMK_ROWS_IRRIGATION};

// the limit's launch, right behind the irrigation's on the same stream whenever the limit is on
static void irrsup_launch(elmk_ctx* ctx, int idt)
{
  if (!ctx->irrsup_rows) return;
  const elmk_ctx::Routing& T = ctx->route;
  const CsrMap& M = ctx->ogrid.map;
  launch_irrigation_supply(ctx->ncols, ctx->irr_rows, ctx->ld, idt, OGridMap{M.ptr, M.col, M.w, M.nrows, 0.0}, T.area,
                           T.rows + (size_t)ROUTE_VOLR * (size_t)T.cld, ctx->irrsup_thr, ctx->irrsup_rows, T.cld, ctx->stream, T.dam.rows,
                           T.dam.tab,  // (D7 while the reservoirs are on)
                           T.cmd.mem ? T.cmd_dam : nullptr, T.cmd.mem ? T.cmd.tab + (size_t)CMD_NDEP * (size_t)T.cld : nullptr);  // (C6)
}

void irr_run_launch(elmk_ctx* ctx, double dt)
{
  if (!hyd_land(ctx)) return;
  launch_irrigation_run(ctx->d, ctx->ncols, ctx->irr_rows, ctx->irr_sched, (int)dt, ctx->run.table, ctx->run.cursor, ctx->stream);
  irrsup_launch(ctx, (int)dt);
}

int irrsup_holds(elmk_ctx* ctx, const char* who)
{
  if (!ctx->irrsup_rows) return ELMK_OK;
  return invalid(ctx, (std::string(who) + ": the irrigation's river supply limit is on (elmk_irrigation_supply_clear first)").c_str());
}
}  // namespace elmk

namespace {
constexpr const Rows& IRR = ROWS_OF_IRRIGATION;
constexpr int IRRSUP_NROWS = 4;
static_assert(ELMK_IRRSUP_DEMAND == 0 && ELMK_IRRSUP_UNMET_SUM == IRRSUP_NROWS - 1, "four rows");

int irrsup_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  return ctx->irrsup_rows ? ELMK_OK : invalid(ctx, (std::string(who) + ": not enabled (elmk_irrigation_supply_enable)").c_str());
}
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
  if (hyd_land(ctx)) {
    launch_irrigation(ctx->d, ctx->ncols, ctx->irr_rows, ctx->irr_sched, (int)dt, tod_seconds, ctx->stream);
    irrsup_launch(ctx, (int)dt);
  }
  return launched(ctx);
}

int elmk_irrigation_read(elmk_ctx* ctx, int w, double* host, int64_t col0, int64_t n) { return rows_read(ctx, IRR, "elmk_irrigation_read", w, host, col0, n); }

int elmk_irrigation_clear(elmk_ctx* ctx)
{
  if (ctx && ctx->irr_rows) {
    if (int rc = irrsup_holds(ctx, "elmk_irrigation_clear")) return rc;       // (the limit reads and scales RATE)
    if (int rc = route_holds(ctx, "elmk_irrigation_clear", true)) return rc;  // (the withdrawal reads QFLX_IRRIG)
  }
  const int rc = rows_clear(ctx, IRR, "elmk_irrigation_clear");
  if (rc == ELMK_OK && !ctx->irr_rows) ctx->irr_sched = nullptr;
  return rc;
}

int elmk_irrigation_supply_enable(elmk_ctx* ctx, double threshold)
{
  const char* who = "elmk_irrigation_supply_enable";
  if (int rc = enter(ctx)) return rc;
  if (!ctx->irr_rows) return invalid(ctx, "elmk_irrigation_supply_enable: the irrigation is not enabled (elmk_irrigation_enable)");
  if (!ctx->route.mem) return invalid(ctx, "elmk_irrigation_supply_enable: runoff routing is not enabled (elmk_routing_enable)");
  if (!ctx->route.withdraw) return invalid(ctx, "elmk_irrigation_supply_enable: the withdrawal is off (elmk_routing_set_withdrawal)");
  if (!(std::isfinite(threshold) && threshold >= 0.0 && threshold < 1.0))
    return invalid(ctx, "elmk_irrigation_supply_enable: threshold not finite and in [0, 1)");
  if (ctx->irrsup_rows) return invalid(ctx, "elmk_irrigation_supply_enable: already enabled");
  if (int rc = refuse_capture(ctx, who)) return rc;
  // every column in at most one cell: the context keeps no host copy of the output grid's map, so from a download of its col
  const CsrMap& M = ctx->ogrid.map;
  std::vector<int32_t> col((size_t)M.nnz);
  if (M.nnz > 0) HIPCHK(hipMemcpyAsync(col.data(), M.col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (const int64_t shared = csr_shared_column(ctx->ncols, M.nnz, col.data()); shared != -1)
    return invalid(ctx, (std::string(who) + ": column " + std::to_string(shared) +
                         " is in more than one cell of the output grid (or twice in one)").c_str());
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its moment)
  const size_t bytes = (size_t)IRRSUP_NROWS * (size_t)ctx->route.cld * sizeof(double);
  if (hip_fail(ctx, ctx->irrsup_rows.alloc(bytes), "hipMalloc(irrigation supply rows)")) return ELMK_E_NOMEM;
  if (hip_fail(ctx, hipMemsetAsync(ctx->irrsup_rows, 0, bytes, ctx->stream), "hipMemset(irrigation supply rows)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->irrsup_rows.reset();
    return ELMK_E_HIP;
  }
  ctx->irrsup_thr = threshold;
  return ELMK_OK;
}

int elmk_irrigation_supply_init(elmk_ctx* ctx, const double* unmet_sum)
{
  const char* who = "elmk_irrigation_supply_init";
  if (int rc = irrsup_enter(ctx, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  const size_t cld = (size_t)ctx->route.cld, n = (size_t)ctx->route.ncells;
  HIPCHK(hipMemsetAsync(ctx->irrsup_rows, 0, (size_t)IRRSUP_NROWS * cld * sizeof(double), ctx->stream));
  if (unmet_sum) HIPCHK(hipMemcpyAsync(ctx->irrsup_rows + ELMK_IRRSUP_UNMET_SUM * cld, unmet_sum, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_irrigation_supply_read(elmk_ctx* ctx, int which, double* host, int64_t cell0, int64_t n)
{
  const char* who = "elmk_irrigation_supply_read";
  if (int rc = irrsup_enter(ctx, who)) return rc;
  if (which < 0 || which >= IRRSUP_NROWS) return invalid(ctx, "elmk_irrigation_supply_read: unknown row");
  if (int rc = check_range(ctx, who, host, cell0, n, ctx->route.ncells, "cell")) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->irrsup_rows + (size_t)which * (size_t)ctx->route.cld + (size_t)cell0, (size_t)n * 8,
                          hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int elmk_irrigation_supply_reset(elmk_ctx* ctx)
{
  if (int rc = irrsup_enter(ctx, "elmk_irrigation_supply_reset")) return rc;
  const size_t cld = (size_t)ctx->route.cld;
  HIPCHK(hipMemsetAsync(ctx->irrsup_rows + ELMK_IRRSUP_UNMET_SUM * cld, 0, cld * sizeof(double), ctx->stream));
  return ELMK_OK;
}

int elmk_irrigation_supply_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_irrigation_supply_clear")) return rc;
  if (!ctx->irrsup_rows) return ELMK_OK;
  if (int rc = cellrows_hold(ctx, "elmk_irrigation_supply_clear", ELMK_CELL_ROWS_SUPPLY, 0, IRRSUP_NROWS - 1)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  (void)ctx->irrsup_rows.reset();
  ctx->irrsup_thr = 0.0;
  return ELMK_OK;
}

}  // extern "C"
