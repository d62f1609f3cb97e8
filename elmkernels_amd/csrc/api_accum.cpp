// api_accum.cpp - accumulated fields (k_accum.hip; include/elmk.h "accumulated fields").
#include "elmk_ctx.h"

namespace {
constexpr int ACCUM_MAX_ROWS = ELMK_ACCUM_MAX_ENTRIES * MAXLEV_STAGE;
constexpr size_t ACCUM_COUNTS_OFF = ((size_t)ACCUM_MAX_ROWS * sizeof(AccumRow) + 255) / 256 * 256;
constexpr size_t ACCUM_TABLE_BYTES = ACCUM_COUNTS_OFF + 256;
static_assert(ELMK_ACCUM_MAX_ENTRIES * sizeof(unsigned long long) <= 256, "the counts fit behind the rows");

}  // namespace

namespace elmk {
unsigned long long* accum_counts(elmk_ctx* ctx) { return (unsigned long long*)((char*)ctx->accum_table + ACCUM_COUNTS_OFF); }

// every row of every entry, then the counts (two launches; nothing without entries)
void accum_update_launch(elmk_ctx* ctx)
{
  launch_accum_update((const AccumRow*)(char*)ctx->accum_table, (int)ctx->accum_rows.size(), accum_counts(ctx), (int)ctx->accum.size(),
                      ctx->ncols, ctx->stream);
}
}  // namespace elmk

extern "C" {

int elmk_accum_add(elmk_ctx* ctx, int src_field, int kind, int64_t period_steps, int dst_field)
{
  if (int rc = enter(ctx)) return rc;
  if (!field_ok(src_field)) return invalid(ctx, "elmk_accum_add: unknown source field");
  if (kind < ELMK_ACCUM_RUNMEAN || kind > ELMK_ACCUM_RUNACCUM) return invalid(ctx, "elmk_accum_add: unknown kind");
  if (period_steps < 1) return invalid(ctx, "elmk_accum_add: the period must be at least one step");
  const int nlev = g_fields[src_field].nlev;
  if (dst_field != -1) {
    if (!field_ok(dst_field)) return invalid(ctx, "elmk_accum_add: unknown destination field");
    if (g_fields[dst_field].dtype != ELMK_F64 || g_fields[dst_field].nlev != nlev)
      return invalid(ctx, "elmk_accum_add: the destination must be an F64 field of the source's levels");
    if (field_class(dst_field) != ELMK_CLASS_SURFACE)
      return invalid(ctx, "elmk_accum_add: the destination must be of class SURFACE (no kernel of the step may write it)");
    if (dst_field == src_field) return invalid(ctx, "elmk_accum_add: the destination is the entry's own source");
    for (const elmk_ctx::AccumEntry& e : ctx->accum) {
      if (e.dst == dst_field) return invalid(ctx, "elmk_accum_add: the field is the destination of another entry");
      // all rows run in one launch: a row reading what another row writes would see old or new values, element by element
      if (e.src == dst_field) return invalid(ctx, "elmk_accum_add: the destination is the source of another entry");
    }
  }
  for (const elmk_ctx::AccumEntry& e : ctx->accum)
    if (e.dst == src_field) return invalid(ctx, "elmk_accum_add: the source is the destination of another entry");
  if ((int)ctx->accum.size() >= ELMK_ACCUM_MAX_ENTRIES) return invalid(ctx, "elmk_accum_add: the accumulator table is full");
  if (int rc = refuse_capture(ctx, "elmk_accum_add")) return rc;
  const bool first = !ctx->accum_table;
  if (first) {
    if (hip_fail(ctx, ctx->accum_table.alloc(ACCUM_TABLE_BYTES), "hipMalloc(accumulator table)")) return ELMK_E_NOMEM;
    if (hip_fail(ctx, hipMemsetAsync(ctx->accum_table, 0, ACCUM_TABLE_BYTES, ctx->stream), "hipMemset(accumulator table)")) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)ctx->accum_table.reset();
      return ELMK_E_HIP;
    }
  }
  const size_t bytes = (size_t)nlev * (size_t)ctx->ld * sizeof(double);
  DevBuf<double> val;
  if (hip_fail(ctx, val.alloc(bytes), "hipMalloc(accumulator)")) {
    if (first) (void)ctx->accum_table.reset();  // the table is held exactly while entries exist
    return ELMK_E_NOMEM;
  }
  const int entry = (int)ctx->accum.size(), row0 = (int)ctx->accum_rows.size();
  const int ses = store_size(g_fields[src_field].dtype);
  for (int l = 0; l < nlev; l++) {
    const size_t row = (size_t)l * (size_t)ctx->ld;
    ctx->accum_rows.push_back(AccumRow{(const char*)ctx->fptr[src_field] + row * ses, val + row,
                                       dst_field >= 0 ? (char*)ctx->fptr[dst_field] + row * store_size(ELMK_F64) : nullptr, period_steps,
                                       store_dtype(g_fields[src_field].dtype), kind, entry, kStateF32 ? 1 : 0});
  }
  // the stream may still run an update that reads the table: the copies are ordered after it; pageable source, so wait
  const unsigned long long zero = 0;
  hipError_t e = hipMemsetAsync(val, 0, bytes, ctx->stream);
  if (!e) e = hipMemcpyAsync((AccumRow*)(char*)ctx->accum_table + row0, &ctx->accum_rows[row0], (size_t)nlev * sizeof(AccumRow),
                             hipMemcpyHostToDevice, ctx->stream);
  if (!e) e = hipMemcpyAsync(accum_counts(ctx) + entry, &zero, sizeof zero, hipMemcpyHostToDevice, ctx->stream);
  if (!e) e = hipStreamSynchronize(ctx->stream);
  if (hip_fail(ctx, e, "elmk_accum_add")) {
    ctx->accum_rows.resize(row0);
    (void)hipStreamSynchronize(ctx->stream);
    if (first) (void)ctx->accum_table.reset();
    return ELMK_E_HIP;  // (frees val)
  }
  ctx->accum.push_back(elmk_ctx::AccumEntry{src_field, kind, dst_field, nlev, row0, period_steps, std::move(val)});
  ctx->accum_version++;
  return entry;
}

int elmk_accum_init(elmk_ctx* ctx, int entry, const double* host, int64_t nsteps)
{
  if (int rc = enter(ctx)) return rc;
  if (entry < 0 || entry >= (int)ctx->accum.size()) return invalid(ctx, "elmk_accum_init: unknown entry");
  if (nsteps < 0) return invalid(ctx, "elmk_accum_init: nsteps must not be negative");
  const elmk_ctx::AccumEntry& e = ctx->accum[entry];
  if (!host && e.dst < 0) return invalid(ctx, "elmk_accum_init: no host values and no destination field to seed from");
  if (int rc = refuse_capture(ctx, "elmk_accum_init")) return rc;
  if (host) {
    if (ctx->ncols > 0)
      if (int rc = xfer_rows(ctx, (char*)(double*)e.val, ctx->ld, 8, e.nlev, const_cast<double*>(host), 0, ctx->ncols, ELMK_LAYOUT_SOA, true)) return rc;
  } else {
    launch_accum_seed(ctx->fptr[e.dst], store_dtype(ELMK_F64), e.val, e.nlev, ctx->ld, ctx->ncols, ctx->stream);
    HIPCHK(hipGetLastError());
  }
  const unsigned long long n = (unsigned long long)nsteps;
  HIPCHK(hipMemcpyAsync(accum_counts(ctx) + entry, &n, sizeof n, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_accum_update(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->accum.empty()) return ELMK_OK;
  accum_update_launch(ctx);
  return launched(ctx);
}

int elmk_accum_read(elmk_ctx* ctx, int entry, double* host, int64_t col0, int64_t n, int layout, int64_t* nsteps)
{
  if (int rc = enter(ctx)) return rc;
  if (entry < 0 || entry >= (int)ctx->accum.size()) return invalid(ctx, "elmk_accum_read: unknown entry");
  if (int rc = check_range(ctx, "elmk_accum_read", host, col0, n, ctx->ncols)) return rc;
  if (layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR) return invalid(ctx, "elmk_accum_read: unknown layout");
  if (int rc = refuse_capture(ctx, "elmk_accum_read")) return rc;
  const elmk_ctx::AccumEntry& e = ctx->accum[entry];
  unsigned long long cnt = 0;
  HIPCHK(hipMemcpyAsync(&cnt, accum_counts(ctx) + entry, sizeof cnt, hipMemcpyDeviceToHost, ctx->stream));
  if (n > 0)
    if (int rc = xfer_rows(ctx, (char*)(double*)e.val, ctx->ld, 8, e.nlev, host, col0, n, layout, false)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (the count and the rows)
  if (nsteps) *nsteps = (int64_t)cnt;
  return ELMK_OK;
}

int elmk_accum_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_accum_clear")) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->accum.empty()) return ELMK_OK;
  ctx->accum.clear();
  ctx->accum_rows.clear();
  HIPCHK(ctx->accum_table.reset());
  ctx->accum_version++;
  return ELMK_OK;
}

}  // extern "C"
