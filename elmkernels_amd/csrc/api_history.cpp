// api_history.cpp - history tapes, the output grid and gridded history entries (k_history.hip; include/elmk.h "history", "output grid").
#include "elmk_ctx.h"

namespace {
constexpr int HIST_MAX_ROWS = ELMK_HIST_MAX_ENTRIES * MAXLEV_STAGE;
constexpr size_t HIST_COUNTS_OFF = ((size_t)HIST_MAX_ROWS * sizeof(HistRow) + 255) / 256 * 256;
constexpr size_t HIST_CROWS_OFF = HIST_COUNTS_OFF + 256;  // the cell rows of gridded entries
constexpr size_t HIST_TABLE_BYTES = HIST_CROWS_OFF + (size_t)HIST_MAX_ROWS * sizeof(HistRow);
static_assert(ELMK_HIST_MAX_TAPES * sizeof(unsigned long long) <= 256, "the counts fit before the cell rows");

HistRow* hist_cell_rows(elmk_ctx* ctx) { return (HistRow*)((char*)(HistRow*)ctx->hist_table + HIST_CROWS_OFF); }

OGridMap ogrid_map(const elmk_ctx* ctx)
{
  const CsrMap& M = ctx->ogrid.map;
  return OGridMap{M.ptr, M.col, M.w, M.nrows, ctx->ogrid.fill};
}

bool has_gridded_entries(const elmk_ctx* ctx) { return !ctx->hist_crows.empty(); }

bool tape_ok(int tape) { return tape >= 0 && tape < ELMK_HIST_MAX_TAPES; }

}  // namespace

namespace elmk {
// the rows of a cell-row family (ELMK_CELL_ROWS_*) for a history or point-series entry: the device row `which` over the routing's cells, or null with
// *why set - exactly the rows elmk_routing_read / elmk_irrigation_supply_read accept at this moment
const double* cell_row(const elmk_ctx* ctx, int family, int which, const char** why)
{
  if (family == ELMK_CELL_ROWS_ROUTING) return route_row(ctx, which, why);
  if (family != ELMK_CELL_ROWS_SUPPLY) return *why = "unknown cell-row family", nullptr;
  if (!ctx->irrsup_rows) return *why = "the irrigation's river supply limit is not on (elmk_irrigation_supply_enable)", nullptr;
  if (which < ELMK_IRRSUP_DEMAND || which > ELMK_IRRSUP_UNMET_SUM) return *why = "row out of range", nullptr;
  return ctx->irrsup_rows + (size_t)which * (size_t)ctx->route.cld;
}

unsigned long long* hist_counts(elmk_ctx* ctx) { return (unsigned long long*)((char*)(HistRow*)ctx->hist_table + HIST_COUNTS_OFF); }

unsigned hist_tape_mask(const elmk_ctx* ctx)
{
  unsigned m = 0;
  for (const elmk_ctx::HistEntry& e : ctx->hist) m |= 1u << e.tape;
  return m;
}

// the tapes of mask hold samples: elmk_history_add refuses them until their reset
int hist_has_family(const elmk_ctx* ctx, int family)
{
  for (const elmk_ctx::HistEntry& e : ctx->hist)
    if (e.family == family) return 1;
  return 0;
}

int cellrows_hold(elmk_ctx* ctx, const char* who, int family, int which0, int which1)
{
  for (const elmk_ctx::HistEntry& e : ctx->hist) {
    if (!e.cellrow) continue;
    const int which = e.field & 0xFFFF;  // (ELMK_RESTART_ROW_FIELD)
    if (family < 0 || (e.family == ELMK_ROWS_NFAMILY + family && which >= which0 && which <= which1))
      return invalid(ctx, (std::string(who) + ": cell-row history entries exist on its rows (elmk_history_clear first)").c_str());
  }
  return points_hold_cellrows(ctx, who, family, which0, which1);
}

void mark_sampled(elmk_ctx* ctx, unsigned mask)
{
  for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++)
    if (mask & (1u << t)) ctx->hist_dirty[t] = true;
}

// every row of every tape, one launch: the column rows alone as before any gridded entry existed, else with the cell rows after them
void hist_accumulate_launch(elmk_ctx* ctx)
{
  const unsigned mask = hist_tape_mask(ctx);
  if (!ctx->hist_rrows.empty())  // cell-row entries: the third kernel, which folds every kind of row
    launch_hist_accumulate_rows(ctx->hist_table, (int)ctx->hist_rows.size(), hist_cell_rows(ctx), (int)ctx->hist_crows.size(), ctx->hist_rtable,
                                (int)ctx->hist_rrows.size(), ogrid_map(ctx), hist_counts(ctx), ctx->ncols, mask, ctx->stream);
  else if (!has_gridded_entries(ctx))
    launch_hist_accumulate(ctx->hist_table, (int)ctx->hist_rows.size(), hist_counts(ctx), ctx->ncols, mask, ctx->stream);
  else
    launch_hist_accumulate_cells(ctx->hist_table, (int)ctx->hist_rows.size(), hist_cell_rows(ctx), (int)ctx->hist_crows.size(),
                                 ogrid_map(ctx), hist_counts(ctx), ctx->ncols, mask, ctx->stream);
}
}  // namespace elmk

namespace {
// elmk_history_add (cells = false: accumulators over the columns) and elmk_gridded_history_add (cells = true: over the output grid's
// cells); `who` names the entry point in the messages.  family >= 0 (elmk_column_history_add_row, elmk_gridded_history_add_row): the entry
// samples row `field` of that feature family instead of a state field: one level, true fp64 in both builds
// cfamily >= 0 (elmk_cell_history_add_row): the entry samples cell row `field` of that cell-row family, a row over the output grid's cells
// that is its own sample: one level, accumulators over the cells, no map and no fill
int hist_add(elmk_ctx* ctx, int tape, int field, int op, bool cells, const char* who, int family = -1, int cfamily = -1)
{
  if (int rc = enter(ctx)) return rc;
  const std::string w = who;
  if (!tape_ok(tape)) return invalid(ctx, (w + ": unknown tape").c_str());
  const bool cellrow = cfamily >= 0, row = family >= 0 || cellrow;
  const double* frow = nullptr;
  if (row) {
    const char* why = nullptr;
    frow = cellrow ? cell_row(ctx, cfamily, field, &why) : feature_row(ctx, family, field, &why);
    if (!frow) return invalid(ctx, (w + ": " + why).c_str());
  } else if (!field_ok(field)) {
    return invalid(ctx, (w + ": unknown field").c_str());
  }
  if (op < ELMK_HIST_AVG || op > ELMK_HIST_INST) return invalid(ctx, (w + ": unknown op").c_str());
  if (cells && !ctx->ogrid.mem) return invalid(ctx, (w + ": no output grid (elmk_set_output_grid)").c_str());
  if ((int)ctx->hist.size() >= ELMK_HIST_MAX_ENTRIES) return invalid(ctx, (w + ": the history table is full").c_str());
  if (ctx->hist_dirty[tape]) return invalid(ctx, (w + ": the tape holds samples; reset it first").c_str());
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (!ctx->hist_table) {
    HIPCHK(ctx->hist_table.alloc(HIST_TABLE_BYTES));
    HIPCHK(hipMemsetAsync(ctx->hist_table, 0, HIST_TABLE_BYTES, ctx->stream));
  }
  if (cellrow && !ctx->hist_rtable) {  // (one level per entry: ELMK_HIST_MAX_ENTRIES rows at the most)
    HIPCHK(ctx->hist_rtable.alloc((size_t)ELMK_HIST_MAX_ENTRIES * sizeof(HistRow)));
    HIPCHK(hipMemsetAsync(ctx->hist_rtable, 0, (size_t)ELMK_HIST_MAX_ENTRIES * sizeof(HistRow), ctx->stream));
  }
  const int nlev = row ? 1 : g_fields[field].nlev;
  // a column row spans the level stride; a cell row the cell count rounded up to 64 (16-byte aligned rows for k_hist_reset's pairs)
  const int64_t ld = cellrow ? ctx->route.cld : cells ? (ctx->ogrid.map.nrows + 63) / 64 * 64 : ctx->ld;
  const size_t bytes = (size_t)nlev * (size_t)ld * sizeof(double);
  DevBuf<double> acc;
  if (hip_fail(ctx, acc.alloc(bytes), "hipMalloc(history)")) return ELMK_E_NOMEM;
  launch_fill(acc, ELMK_F64, nlev, ld, ld, hist_init_value(op), ctx->stream);
  std::vector<HistRow>& rows = cellrow ? ctx->hist_rrows : cells ? ctx->hist_crows : ctx->hist_rows;
  HistRow* table = cellrow ? (HistRow*)ctx->hist_rtable : cells ? hist_cell_rows(ctx) : (HistRow*)ctx->hist_table;
  const int row0 = (int)rows.size();
  if (row) {
    rows.push_back(HistRow{frow, acc, ELMK_F64, op, tape, cellrow ? 1 : 0});  // (pad: 1 marks a cell-row entry's row)
  } else {
    const int es = store_size(g_fields[field].dtype);
    for (int l = 0; l < nlev; l++)
      rows.push_back(HistRow{(const char*)ctx->fptr[field] + (size_t)l * (size_t)ctx->ld * es, acc + (size_t)l * (size_t)ld,
                             store_dtype(g_fields[field].dtype), op, tape, 0});
  }
  // the stream may still run an accumulate that reads the table: the copy is ordered after it; pageable source, so wait
  const hipError_t e1 = hipGetLastError();
  const hipError_t e2 = e1 == hipSuccess ? hipMemcpyAsync(table + row0, &rows[row0], (size_t)nlev * sizeof(HistRow), hipMemcpyHostToDevice,
                                                          ctx->stream)
                                         : e1;
  const hipError_t e3 = e2 == hipSuccess ? hipStreamSynchronize(ctx->stream) : e2;
  if (hip_fail(ctx, e3, who)) {
    rows.resize(row0);
    (void)hipStreamSynchronize(ctx->stream);
    return ELMK_E_HIP;  // (frees acc)
  }
  if (cellrow) family = ELMK_ROWS_NFAMILY + cfamily;
  ctx->hist.push_back(elmk_ctx::HistEntry{tape, row ? ELMK_RESTART_ROW_FIELD(family, field) : field, op, nlev, row0, std::move(acc), cells, ld, family,
                                          cellrow});
  ctx->hist_version++;
  return (int)ctx->hist.size() - 1;
}
}  // namespace

extern "C" {

int elmk_history_add(elmk_ctx* ctx, int tape, int field, int op) { return hist_add(ctx, tape, field, op, false, "elmk_history_add"); }

int elmk_column_history_add_row(elmk_ctx* ctx, int tape, int family, int which, int op)
{
  if (family < 0) return ctx ? invalid(ctx, "elmk_column_history_add_row: unknown row family") : ELMK_E_INVALID;
  return hist_add(ctx, tape, which, op, false, "elmk_column_history_add_row", family);
}

int elmk_history_accumulate(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->hist.empty()) return ELMK_OK;
  hist_accumulate_launch(ctx);
  HIPCHK(hipGetLastError());
  mark_sampled(ctx, hist_tape_mask(ctx));
  return ELMK_OK;
}

int elmk_history_reset(elmk_ctx* ctx, int tape)
{
  if (int rc = enter(ctx)) return rc;
  if (!tape_ok(tape)) return invalid(ctx, "elmk_history_reset: unknown tape");
  if (ctx->hist_table) {
    launch_hist_reset(ctx->hist_table, (int)ctx->hist_rows.size(), hist_counts(ctx), ctx->ncols, tape, ctx->stream);
    HIPCHK(hipGetLastError());
  }
  if (has_gridded_entries(ctx)) {  // (resets the tape's count a second time)
    launch_hist_reset(hist_cell_rows(ctx), (int)ctx->hist_crows.size(), hist_counts(ctx), (ctx->ogrid.map.nrows + 63) / 64 * 64, tape,
                      ctx->stream);
    HIPCHK(hipGetLastError());
  }
  if (!ctx->hist_rrows.empty()) {  // (and once more)
    launch_hist_reset(ctx->hist_rtable, (int)ctx->hist_rrows.size(), hist_counts(ctx), ctx->route.cld, tape, ctx->stream);
    HIPCHK(hipGetLastError());
  }
  ctx->hist_dirty[tape] = false;
  return ELMK_OK;
}

int elmk_history_count(elmk_ctx* ctx, int tape, int64_t* nsamples)
{
  if (int rc = enter(ctx)) return rc;
  if (!tape_ok(tape) || !nsamples) return invalid(ctx, "elmk_history_count: bad arguments");
  unsigned long long c = 0;
  if (ctx->hist_table)
    HIPCHK(hipMemcpyAsync(&c, hist_counts(ctx) + tape, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  *nsamples = (int64_t)c;
  return ELMK_OK;
}

int elmk_history_read(elmk_ctx* ctx, int entry, double* host, int64_t col0, int64_t n, int layout)
{
  if (int rc = enter(ctx)) return rc;
  if (entry < 0 || entry >= (int)ctx->hist.size()) return invalid(ctx, "elmk_history_read: unknown entry");
  const elmk_ctx::HistEntry& e = ctx->hist[entry];
  // a gridded entry's col0, n index cells, and so do a cell-row entry's (one level: the layout says nothing and is not looked at)
  const int64_t lim = e.cellrow ? ctx->route.ncells : e.cells ? ctx->ogrid.map.nrows : ctx->ncols;
  if (int rc = check_range(ctx, "elmk_history_read", host, col0, n, lim, e.cells || e.cellrow ? "cell" : "column")) return rc;
  if (!e.cellrow && layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR) return invalid(ctx, "elmk_history_read: unknown layout");
  int64_t count = 0;
  if (int rc = elmk_history_count(ctx, e.tape, &count)) return rc;
  if (count <= 0) return invalid(ctx, "elmk_history_read: the tape holds no samples");
  if (n == 0) return ELMK_OK;
  // chunks of m columns: the finalize kernel writes them as dense SoA [lev][m] into the upper half of the staging buffer, and the
  // transpose of elmk_download takes them to [col][lev] in the lower half where the caller wants the reference layout
  const size_t half = ctx->staging.bytes() / 2 / sizeof(double) * sizeof(double);
  const int64_t chunk = (int64_t)(half / ((size_t)e.nlev * sizeof(double)));
  if (chunk <= 0) return invalid(ctx, "staging buffer too small");
  double* soa = (double*)(ctx->staging + half);
  for (int64_t done = 0; done < n; done += chunk) {
    const int64_t m = (n - done) < chunk ? (n - done) : chunk;
    if (e.cells)
      launch_ogrid_finalize(e.acc, e.cld, e.nlev, e.op, count, ctx->ogrid.map.ptr, ctx->ogrid.fill, col0 + done, m, soa, ctx->stream);
    else
      launch_hist_finalize(e.acc, e.cellrow ? e.cld : ctx->ld, e.nlev, e.op, count, col0 + done, m, soa, ctx->stream);
    if (layout == ELMK_LAYOUT_SOA || e.nlev == 1) {
      HIPCHK(hipMemcpy2DAsync(host + done, (size_t)n * sizeof(double), soa, (size_t)m * sizeof(double), (size_t)m * sizeof(double),
                              e.nlev, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      launch_soa_to_cols(soa, ctx->staging, 8, e.nlev, m, 0, m, ctx->stream);
      HIPCHK(hipMemcpyAsync(host + (size_t)done * e.nlev, ctx->staging, (size_t)m * e.nlev * sizeof(double), hipMemcpyDeviceToHost,
                            ctx->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));  // staging is reused by the next chunk
  }
  return ELMK_OK;
}

int elmk_history_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->hist.clear();
  ctx->hist_rows.clear();
  ctx->hist_crows.clear();
  ctx->hist_rrows.clear();
  if (ctx->hist_table)
    HIPCHK(hipMemsetAsync(hist_counts(ctx), 0, ELMK_HIST_MAX_TAPES * sizeof(unsigned long long), ctx->stream));
  for (bool& d : ctx->hist_dirty) d = false;
  ctx->hist_version++;
  return synced(ctx);
}

// ---------------------------------------------------------------------------------------------------
// output grid: columns aggregated onto cells on the device through a CSR map (include/elmk.h "output grid")
// ---------------------------------------------------------------------------------------------------
int elmk_set_output_grid(elmk_ctx* ctx, int64_t ncells, const int64_t* ptr, const int32_t* col, const double* w, double fill)
{
  if (int rc = enter(ctx)) return rc;
  // (every gather of the aggregate kernels stays inside a source row because of this check)
  if (int rc = invalid_map(ctx, "elmk_set_output_grid", csr_check(ncells, ctx->ncols, ptr, col, w, "ncells outside 1 .. 2^31-1", false, false))) return rc;
  if (int rc = refuse_capture(ctx, "elmk_set_output_grid")) return rc;
  if (has_gridded_entries(ctx)) return invalid(ctx, "elmk_set_output_grid: gridded history entries exist (elmk_history_clear first)");
  if (int rc = cellrows_hold(ctx, "elmk_set_output_grid")) return rc;  // (ncells is the grid's)
  if (int rc = points_hold_grid(ctx, "elmk_set_output_grid")) return rc;
  if (int rc = irrsup_holds(ctx, "elmk_set_output_grid")) return rc;
  if (int rc = land_holds(ctx, "elmk_set_output_grid")) return rc;
  if (int rc = route_holds(ctx, "elmk_set_output_grid")) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (a gridded download may still read the old map)
  elmk_ctx::OGrid& O = ctx->ogrid;
  O = elmk_ctx::OGrid{};
  O.fill = fill;
  const int rc = hip_fail(ctx, carve(O.mem, [&](Carve& L) { O.map.take(L, ncells, ptr[ncells]); }), "hipMalloc(output grid)")
                     ? ELMK_E_NOMEM
                     : O.map.upload(ctx, ptr, col, w, [] { return false; });
  if (rc != ELMK_OK) O = elmk_ctx::OGrid{};
  return rc;
}

int elmk_clear_output_grid(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_clear_output_grid")) return rc;
  if (has_gridded_entries(ctx)) return invalid(ctx, "elmk_clear_output_grid: gridded history entries exist (elmk_history_clear first)");
  if (int rc = cellrows_hold(ctx, "elmk_clear_output_grid")) return rc;
  if (int rc = points_hold_grid(ctx, "elmk_clear_output_grid")) return rc;
  if (int rc = irrsup_holds(ctx, "elmk_clear_output_grid")) return rc;
  if (int rc = land_holds(ctx, "elmk_clear_output_grid")) return rc;
  if (int rc = route_holds(ctx, "elmk_clear_output_grid")) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->ogrid = elmk_ctx::OGrid{};
  return ELMK_OK;
}

int elmk_download_gridded(elmk_ctx* ctx, int field, int level, double* cells)
{
  if (int rc = enter(ctx)) return rc;
  const elmk_ctx::OGrid& O = ctx->ogrid;
  if (!O.mem) return invalid(ctx, "elmk_download_gridded: no output grid (elmk_set_output_grid)");
  if (!field_ok(field)) return invalid(ctx, "elmk_download_gridded: unknown field");
  if (level < 0 || level >= g_fields[field].nlev) return invalid(ctx, "elmk_download_gridded: level out of range");
  if (!cells) return invalid(ctx, "elmk_download_gridded: null cells");
  if (int rc = refuse_capture(ctx, "elmk_download_gridded")) return rc;
  const int es = store_size(g_fields[field].dtype);
  const char* src = (const char*)ctx->fptr[field] + (size_t)level * (size_t)ctx->ld * es;
  // chunks of cells through the staging buffer, which the next chunk reuses
  const int64_t chunk = (int64_t)(ctx->staging.bytes() / sizeof(double)), ncells = O.map.nrows;
  for (int64_t done = 0; done < ncells; done += chunk) {
    const int64_t m = (ncells - done) < chunk ? (ncells - done) : chunk;
    launch_ogrid_aggregate(src, store_dtype(g_fields[field].dtype), ogrid_map(ctx), done, m, (double*)(char*)ctx->staging, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cells + done, ctx->staging, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  return ELMK_OK;
}

int elmk_gridded_history_add(elmk_ctx* ctx, int tape, int field, int op)
{
  return hist_add(ctx, tape, field, op, true, "elmk_gridded_history_add");
}

int elmk_gridded_history_add_row(elmk_ctx* ctx, int tape, int family, int which, int op)
{
  if (family < 0) return ctx ? invalid(ctx, "elmk_gridded_history_add_row: unknown row family") : ELMK_E_INVALID;
  return hist_add(ctx, tape, which, op, true, "elmk_gridded_history_add_row", family);
}

int elmk_cell_history_add_row(elmk_ctx* ctx, int tape, int family, int which, int op)
{
  if (family < 0 || family >= ELMK_CELL_ROWS_NFAMILY) return ctx ? invalid(ctx, "elmk_cell_history_add_row: unknown cell-row family") : ELMK_E_INVALID;
  return hist_add(ctx, tape, which, op, false, "elmk_cell_history_add_row", -1, family);
}

}  // extern "C"
