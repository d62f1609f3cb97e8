// api_points.cpp - the point series: per-step records of chosen columns and river cells (k_points.hip; include/elmk.h "point series").
#include "elmk_ctx.h"

namespace {
using Points = elmk_ctx::Points;

// The five kinds of entry, said once: which list an entry samples, whether its sample is the output grid's aggregate, whether its source
// is a row (fp64 in both builds) or one level of a state field, and the entry point's name.  The interlocks of P7 and the table the
// kernel reads are derived from these rows.
enum Kind { POINTS_FIELD, POINTS_ROW, POINTS_CELL_ROW, POINTS_GRIDDED_FIELD, POINTS_GRIDDED_ROW, POINTS_NKINDS };
struct KindDesc {
  int list;      // ELMK_POINTS_COLUMNS or ELMK_POINTS_CELLS
  bool gridded;  // the sample is the aggregate over the cell's terms (holds the output grid's map)
  bool row;      // a = family, b = which (else a = field, b = level)
  bool cellrow;  // the row is a cell row (holds the routing's rows and ncells)
  const char* who;
};
constexpr KindDesc KINDS[POINTS_NKINDS] = {
    {ELMK_POINTS_COLUMNS, false, false, false, "elmk_points_add_field"},
    {ELMK_POINTS_COLUMNS, false, true, false, "elmk_points_add_row"},
    {ELMK_POINTS_CELLS, false, true, true, "elmk_points_add_cell_row"},
    {ELMK_POINTS_CELLS, true, false, false, "elmk_points_add_gridded_field"},
    {ELMK_POINTS_CELLS, true, true, false, "elmk_points_add_gridded_row"},
};

int64_t pad8(int64_t n) { return (n + 7) / 8 * 8; }

int refuse(elmk_ctx* ctx, const char* who, const char* text) { return invalid(ctx, (std::string(who) + ": " + text).c_str()); }

// entries and lists may change only before the first record or after a reset (P0)
int config_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->pts.total > 0) return refuse(ctx, who, "the series holds records (elmk_points_reset first)");
  return refuse_capture(ctx, who);
}

int ensure_mem(elmk_ctx* ctx)
{
  Points& P = ctx->pts;
  if (P.mem) return ELMK_OK;
  if (hip_fail(ctx, carve(P.mem, [&](Carve& L) {
                 L.take(P.table, sizeof(PointsTable));
                 L.take(P.base, 256);
                 for (int k = 0; k < ELMK_POINTS_NKIND; k++) L.take(P.dlist[k], (size_t)ELMK_POINTS_MAX_POINTS * sizeof(int64_t));
               }), "hipMalloc(point series)"))
    return ELMK_E_NOMEM;
  HIPCHK(hipMemsetAsync(P.mem, 0, P.mem.bytes(), ctx->stream));
  return ELMK_OK;
}

// why a record cannot be taken now, or null (P4)
const char* not_ready(const elmk_ctx* ctx)
{
  const Points& P = ctx->pts;
  if (P.max_records <= 0) return "no reservation (elmk_points_reserve)";
  if (P.entries.empty()) return "no entries (elmk_points_add_*)";
  for (const Points::Entry& e : P.entries)
    if (P.list[KINDS[e.kind].list].empty())
      return KINDS[e.kind].list == ELMK_POINTS_CELLS ? "an entry's cells list is empty (elmk_points_set)" : "an entry's columns list is empty (elmk_points_set)";
  return nullptr;
}

// After every change of the entries, the lists or the reservation: the layout of a record, the table on the device, and the ring of
// the reservation's size.  The stream is waited for: the sources are host memory, and an earlier ring may still be written.
int push(elmk_ctx* ctx, const char* who)
{
  Points& P = ctx->pts;
  if (int rc = ensure_mem(ctx)) return rc;
  PointsTable T{};
  int64_t out = 0;
  int wave = 0;
  for (size_t k = 0; k < P.entries.size(); k++) {
    const Points::Entry& e = P.entries[k];
    const KindDesc& K = KINDS[e.kind];
    const int n = (int)P.list[K.list].size();
    T.e[k] = PointsEntry{e.src, P.dlist[K.list], out, n, e.dtype, K.gridded ? 1 : 0, wave};
    out += pad8(n);
    wave += K.gridded ? n : (n + 63) / 64;
  }
  T.nentries = (int)P.entries.size();
  T.nwaves = wave;
  P.nwaves = wave;
  P.stride = POINTS_HEAD + out;
  P.version++;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->graph[GRAPH_RUN_STEP].drop();  // (it holds the ring's address)
  const size_t need = (size_t)P.max_records * (size_t)P.stride * sizeof(double);
  if (P.max_records > 0 && P.ring.bytes() != need) {
    if (hip_fail(ctx, P.ring.alloc(need), "hipMalloc(point series ring)")) {
      P.max_records = 0;
      return ELMK_E_NOMEM;
    }
    HIPCHK(hipMemsetAsync(P.ring, 0, need, ctx->stream));
  }
  HIPCHK(hipMemcpyAsync(P.table, &T, sizeof T, hipMemcpyHostToDevice, ctx->stream));
  if (hip_fail(ctx, hipStreamSynchronize(ctx->stream), who)) return ELMK_E_HIP;
  return ELMK_OK;
}

OGridMap points_map(const elmk_ctx* ctx)
{
  const CsrMap& M = ctx->ogrid.map;
  return OGridMap{M.ptr, M.col, M.w, M.nrows, ctx->ogrid.fill};
}

// one source, accepted exactly as the history's entry point of its kind accepts it at this moment (P0)
int add(elmk_ctx* ctx, int kind, int a, int b)
{
  const KindDesc& K = KINDS[kind];
  if (int rc = config_enter(ctx, K.who)) return rc;
  Points& P = ctx->pts;
  const void* src = nullptr;
  int dtype = ELMK_F64;
  if (K.row) {
    const char* why = nullptr;
    if (K.cellrow && (a < 0 || a >= ELMK_CELL_ROWS_NFAMILY)) return refuse(ctx, K.who, "unknown cell-row family");
    if (!K.cellrow && a < 0) return refuse(ctx, K.who, "unknown row family");
    src = K.cellrow ? cell_row(ctx, a, b, &why) : feature_row(ctx, a, b, &why);
    if (!src) return refuse(ctx, K.who, why);
  } else {
    if (!field_ok(a)) return refuse(ctx, K.who, "unknown field");
    if (b < 0 || b >= g_fields[a].nlev) return refuse(ctx, K.who, "level out of range");
    src = (const char*)ctx->fptr[a] + (size_t)b * (size_t)ctx->ld * (size_t)store_size(g_fields[a].dtype);
    dtype = store_dtype(g_fields[a].dtype);
  }
  if (K.gridded && !ctx->ogrid.mem) return refuse(ctx, K.who, "no output grid (elmk_set_output_grid)");
  if ((int)P.entries.size() >= ELMK_POINTS_MAX_ENTRIES) return refuse(ctx, K.who, "the entry table is full");
  P.entries.push_back(Points::Entry{kind, a, b, src, dtype});
  if (int rc = push(ctx, K.who)) {
    P.entries.pop_back();
    return rc;
  }
  return (int)P.entries.size() - 1;
}

// held records are indexed oldest first: record j lies in slot (first + j) % max_records
int64_t first_slot(const Points& P) { return P.total <= P.max_records ? 0 : P.total % P.max_records; }

// nrec records from held index rec0 on: `width` doubles from offset `off` of each slot into host[nrec][width], in at most two copies
int read_slots(elmk_ctx* ctx, const char* who, double* host, int64_t rec0, int64_t nrec, int64_t off, int64_t width)
{
  Points& P = ctx->pts;
  const int64_t held = std::min<int64_t>(P.total, P.max_records);
  if (rec0 < 0 || nrec < 0 || rec0 + nrec > held || (!host && nrec > 0)) return refuse(ctx, who, "bad record range (rec0 + nrec <= held)");
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (nrec > 0 && width > 0) {
    const int64_t s0 = (first_slot(P) + rec0) % P.max_records;
    const int64_t n1 = std::min<int64_t>(nrec, P.max_records - s0);
    const size_t wb = (size_t)width * sizeof(double), sp = (size_t)P.stride * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(host, wb, P.ring + s0 * P.stride + off, sp, wb, (size_t)n1, hipMemcpyDeviceToHost, ctx->stream));
    if (nrec > n1)
      HIPCHK(hipMemcpy2DAsync(host + n1 * width, wb, P.ring + off, sp, wb, (size_t)(nrec - n1), hipMemcpyDeviceToHost, ctx->stream));
  }
  return synced(ctx);
}
}  // namespace

namespace elmk {

int points_hold_family(elmk_ctx* ctx, const char* who, int family)
{
  for (const Points::Entry& e : ctx->pts.entries) {
    const KindDesc& K = KINDS[e.kind];
    if (K.row && !K.cellrow && e.a == family)
      return refuse(ctx, who, "point-series entries over its rows exist (elmk_points_clear first)");
  }
  return ELMK_OK;
}

int points_hold_cellrows(elmk_ctx* ctx, const char* who, int family, int which0, int which1)
{
  for (const Points::Entry& e : ctx->pts.entries) {
    if (!KINDS[e.kind].cellrow) continue;
    if (family < 0 || (e.a == family && e.b >= which0 && e.b <= which1))
      return refuse(ctx, who, "point-series entries over its cell rows exist (elmk_points_clear first)");
  }
  return ELMK_OK;
}

int points_hold_grid(elmk_ctx* ctx, const char* who)
{
  const Points& P = ctx->pts;
  if (!P.list[ELMK_POINTS_CELLS].empty()) return refuse(ctx, who, "the point series holds a cells list (elmk_points_clear first)");
  for (const Points::Entry& e : P.entries)
    if (KINDS[e.kind].list == ELMK_POINTS_CELLS) return refuse(ctx, who, "point-series entries over the grid's cells exist (elmk_points_clear first)");
  return ELMK_OK;
}

int points_run_check(elmk_ctx* ctx)
{
  if (!ctx->pts.run_on) return ELMK_OK;
  if (const char* why = not_ready(ctx)) return invalid(ctx, (std::string("elmk_run: the point series is armed (elmk_points_set_run) with ") + why).c_str());
  return ELMK_OK;
}

int points_run_begin(elmk_ctx* ctx, int buf, const elmk_run_step* steps, int nsteps)
{
  Points& P = ctx->pts;
  const elmk_ctx::Run& R = ctx->run;
  if (P.stamps_steps != R.max_steps) {  // the first armed run of this reservation
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->graph[GRAPH_RUN_STEP].drop();
    P.stamps_steps = 0;
    P.version++;
    const size_t bytes = 2 * (size_t)R.max_steps * sizeof(double);
    if (hip_fail(ctx, P.stamps.alloc(bytes), "hipMalloc(point series stamps)") ||
        hip_fail(ctx, P.stamps_host.alloc(bytes), "hipHostMalloc(point series stamps)"))
      return ELMK_E_NOMEM;
    P.stamps_steps = R.max_steps;
  }
  const int row0 = buf * R.max_steps;
  double* h = P.stamps_host + row0;
  for (int s = 0; s < nsteps; s++) h[s] = steps[s].decday;
  HIPCHK(hipMemcpyAsync(P.stamps + row0, h, (size_t)nsteps * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  // the slot of the step at table row `cursor` is (base + cursor) % max_records: base + row0 = the slot of the run's first record
  const int32_t base = (int32_t)(P.total % P.max_records) - (int32_t)row0;
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)P.base, base, 1, ctx->stream));
  P.total += nsteps;  // (the records are enqueued by the run's steps)
  return ELMK_OK;
}

void points_run_launch(elmk_ctx* ctx)
{
  const Points& P = ctx->pts;
  launch_points_record(P.table, P.nwaves, points_map(ctx), P.ring, P.stride, P.max_records, 0, 0.0, ctx->run.cursor, P.base, P.stamps, ctx->stream);
}

}  // namespace elmk

extern "C" {

int elmk_points_set(elmk_ctx* ctx, int kind, int64_t n, const int64_t* idx)
{
  const char* who = "elmk_points_set";
  if (int rc = config_enter(ctx, who)) return rc;
  if (kind != ELMK_POINTS_COLUMNS && kind != ELMK_POINTS_CELLS) return refuse(ctx, who, "unknown kind");
  if (n < 0 || n > ELMK_POINTS_MAX_POINTS) return refuse(ctx, who, "n outside 0 .. ELMK_POINTS_MAX_POINTS");
  if (n > 0 && !idx) return refuse(ctx, who, "null idx");
  if (kind == ELMK_POINTS_CELLS && !ctx->ogrid.mem) return refuse(ctx, who, "no output grid (elmk_set_output_grid)");
  const int64_t lim = kind == ELMK_POINTS_CELLS ? ctx->ogrid.map.nrows : ctx->ncols;
  for (int64_t i = 0; i < n; i++)  // (every gather of k_points_record stays inside its row because of this check)
    if (idx[i] < 0 || idx[i] >= lim) {
      char text[160];
      snprintf(text, sizeof text, "idx[%lld] = %lld outside 0 .. %s - 1 (%lld)", (long long)i, (long long)idx[i],
               kind == ELMK_POINTS_CELLS ? "ncells" : "ncols", (long long)lim);
      return refuse(ctx, who, text);
    }
  Points& P = ctx->pts;
  if (int rc = ensure_mem(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<int64_t> old(idx, idx + n);
  old.swap(P.list[kind]);
  if (n > 0) HIPCHK(hipMemcpyAsync(P.dlist[kind], idx, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = push(ctx, who)) {
    old.swap(P.list[kind]);
    return rc;
  }
  return ELMK_OK;
}

int elmk_points_add_field(elmk_ctx* ctx, int field, int level) { return add(ctx, POINTS_FIELD, field, level); }
int elmk_points_add_row(elmk_ctx* ctx, int family, int which) { return add(ctx, POINTS_ROW, family, which); }
int elmk_points_add_cell_row(elmk_ctx* ctx, int family, int which) { return add(ctx, POINTS_CELL_ROW, family, which); }
int elmk_points_add_gridded_field(elmk_ctx* ctx, int field, int level) { return add(ctx, POINTS_GRIDDED_FIELD, field, level); }
int elmk_points_add_gridded_row(elmk_ctx* ctx, int family, int which) { return add(ctx, POINTS_GRIDDED_ROW, family, which); }

int elmk_points_reserve(elmk_ctx* ctx, int max_records)
{
  const char* who = "elmk_points_reserve";
  if (int rc = config_enter(ctx, who)) return rc;
  if (max_records < 1 || max_records > (1 << 24)) return refuse(ctx, who, "need 1 <= max_records <= 2^24");
  Points& P = ctx->pts;
  const int old = P.max_records;
  P.max_records = max_records;
  if (int rc = push(ctx, who)) {
    if (P.max_records) P.max_records = old;
    return rc;
  }
  return ELMK_OK;
}

int elmk_points_record(elmk_ctx* ctx, double stamp)
{
  const char* who = "elmk_points_record";
  if (int rc = enter(ctx)) return rc;
  if (const char* why = not_ready(ctx)) return refuse(ctx, who, why);
  if (int rc = refuse_capture(ctx, who)) return rc;
  Points& P = ctx->pts;
  launch_points_record(P.table, P.nwaves, points_map(ctx), P.ring, P.stride, P.max_records, (int)(P.total % P.max_records), stamp, nullptr,
                       nullptr, nullptr, ctx->stream);
  HIPCHK(hipGetLastError());
  P.total++;
  return ELMK_OK;
}

int elmk_points_set_run(elmk_ctx* ctx, int on)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_points_set_run")) return rc;
  Points& P = ctx->pts;
  if (on && P.max_records <= 0) return invalid(ctx, "elmk_points_set_run: no reservation (elmk_points_reserve)");
  P.run_on = on != 0;
  P.version++;
  return ELMK_OK;
}

int elmk_points_count(elmk_ctx* ctx, int64_t* total, int64_t* held)
{
  if (!ctx) return ELMK_E_INVALID;
  const Points& P = ctx->pts;
  if (total) *total = P.total;
  if (held) *held = std::min<int64_t>(P.total, P.max_records);
  return ELMK_OK;
}

int elmk_points_read(elmk_ctx* ctx, int entry, double* host, int64_t rec0, int64_t nrec)
{
  const char* who = "elmk_points_read";
  if (int rc = enter(ctx)) return rc;
  Points& P = ctx->pts;
  if (entry < 0 || entry >= (int)P.entries.size()) return refuse(ctx, who, "unknown entry");
  int64_t off = POINTS_HEAD;
  for (int k = 0; k < entry; k++) off += pad8((int64_t)P.list[KINDS[P.entries[k].kind].list].size());
  return read_slots(ctx, who, host, rec0, nrec, off, (int64_t)P.list[KINDS[P.entries[entry].kind].list].size());
}

int elmk_points_stamps(elmk_ctx* ctx, double* host, int64_t rec0, int64_t nrec)
{
  if (int rc = enter(ctx)) return rc;
  return read_slots(ctx, "elmk_points_stamps", host, rec0, nrec, 0, 1);
}

int elmk_points_reset(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_points_reset")) return rc;
  Points& P = ctx->pts;
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (the records in flight belong to the series that ends here)
  P.total = 0;
  P.run_on = false;
  P.version++;
  return ELMK_OK;
}

int elmk_points_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_points_clear")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  const uint64_t version = ctx->pts.version + 1;
  ctx->pts = Points{};
  ctx->pts.version = version;
  return ELMK_OK;
}

}  // extern "C"
