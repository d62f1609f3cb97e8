// api_restart.cpp - restart images (k_restart.hip; include/elmk.h "restart").
#include "elmk_ctx.h"

namespace {

// the class of every field, from include/elmk_restart.def (-1: not listed, which the static_assert below refuses)
struct ClassTable {
  int c[ELMK_NUM_FIELDS];
  int listed;
};
constexpr ClassTable make_class_table()
{
  ClassTable t{};
  for (int& v : t.c) v = -1;
  t.listed = 0;
#define ELMK_RESTART_CLASS(name, cls) \
  t.c[ELMK_FIELD_##name] = ELMK_CLASS_##cls; \
  t.listed++;
#include "elmk_restart.def"
#undef ELMK_RESTART_CLASS
  return t;
}
constexpr ClassTable g_class = make_class_table();
constexpr bool every_field_classified()
{
  for (int v : g_class.c)
    if (v < 0) return false;
  return g_class.listed == ELMK_NUM_FIELDS;
}
static_assert(every_field_classified(), "include/elmk_restart.def lists every field exactly once");

constexpr size_t RST_ALIGN = 256;
constexpr size_t RST_CHUNK = (size_t)64 << 20;  // bytes of image per staging chunk
constexpr int RST_MAX_PIECES = 8192;            // per chunk (grid.y)
constexpr uint32_t RST_V_ROUTING = ELMK_RESTART_VERSION_ROUTING;
constexpr uint32_t RST_V_RESERVOIR = ELMK_RESTART_VERSION_RESERVOIR;
constexpr uint32_t RST_V_HEAT = ELMK_RESTART_VERSION_HEAT;

uint64_t fmix64(uint64_t k)
{
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

// FNV-1a over name, NUL, dtype, nlev of every field in id order
uint64_t schema_hash()
{
  uint64_t h = 0xcbf29ce484222325ULL;
  auto eat = [&h](unsigned char b) { h = (h ^ b) * 0x100000001b3ULL; };
  for (const FieldDesc& f : g_fields) {
    for (const char* p = f.name; *p; p++) eat((unsigned char)*p);
    eat(0);
    eat((unsigned char)f.dtype);
    eat((unsigned char)f.nlev);
  }
  return h;
}

// the header's checksum: its 8-byte words w_i, header_checksum read as 0, summed as terms of row 0 at position i
uint64_t header_checksum(const unsigned char* img, size_t header_bytes)
{
  uint64_t s = 0;
  for (size_t i = 0; i < header_bytes / 8; i++) {
    uint64_t w;
    memcpy(&w, img + 8 * i, 8);
    if (8 * i == offsetof(elmk_restart_header, header_checksum)) w = 0;
    s += fmix64(w ^ fmix64((uint64_t)i * 64u + 1u));
  }
  return s;
}

struct RstSrc {
  char* dev;      // row 0 on the device
  int64_t ld;     // row stride (elements)
  int sdtype;     // stored type
  int64_t g0;     // global index of element 0
  bool snl;
};

// what an image of this context holds, in order: the section and entry tables and where each section's rows live
struct RstLayout {
  std::vector<elmk_restart_entry> ent;
  std::vector<elmk_restart_accum> acc;  // one per accumulator entry (nsteps filled in by the save)
  std::vector<elmk_restart_section> sec;
  std::vector<RstSrc> src;
  unsigned kinds = 0;    // bit k: the image holds sections of the optional kind k
  uint32_t version = 1;  // the highest introducing version among them; from 2 on the word after the header counts the accumulator entries
  size_t header_bytes = 0, total = 0;
};

// The optional section kinds in image order: the format version that introduced the kind, how many sections this context contributes
// (0: it has not got the feature) and section i's id, levels and rows (F64, ncols wide, the level stride apart), and the feature's name
// and enabling call for the loader's refusals.  An image holds exactly the optional kinds its context has.
struct RstRows {
  int id, nlev;
  double* dev;
};
using Ctx = const elmk_ctx*;
// cells: the kind's sections are rows over the routing's cells (extent ncells, stride cld, g = the cell) and not over the columns;
// implied: an image of the kind's version holds the kind whatever its section table says (every kind that introduced a version)
struct RstKind {
  int kind;
  uint32_t version;
  const char *feature, *enable;
  int (*count)(Ctx);
  RstRows (*rows)(Ctx, int i);
  bool cells = false, implied = true;
};
// (the routing state of version 6, ELMK_OPT_RESTART_CELLS: route_state_rows of api_routing.cpp; with the reservoirs on RES and KRLS
// follow, and the image is of version 7)
const RstKind RST_OPTIONAL[] = {
    {ELMK_RESTART_ACCUM, ELMK_RESTART_VERSION_ACCUM, "accumulator entries", "elmk_accum_add", [](Ctx c) { return (int)c->accum.size(); },
     [](Ctx c, int i) { return RstRows{i, c->accum[i].nlev, c->accum[i].val}; }},
    {ELMK_RESTART_ALT, ELMK_RESTART_VERSION_ALT, "the active layer thickness", "elmk_active_layer_enable",
     [](Ctx c) { return c->alt_rows ? ALT_NROWS : 0; }, [](Ctx c, int i) { return RstRows{i, 1, c->alt_rows + (size_t)i * (size_t)c->ld}; }},
    {ELMK_RESTART_HYDROLOGY, ELMK_RESTART_VERSION_HYDROLOGY, "the soil hydrology", "elmk_soil_hydrology_enable", [](Ctx c) { return c->hyd_rows ? 2 : 0; },
     [](Ctx c, int i) { return RstRows{ELMK_HYD_ZWT + i, 1, c->hyd_rows + (size_t)(ELMK_HYD_ZWT + i) * (size_t)c->ld}; }},
    {ELMK_RESTART_IRRIGATION, ELMK_RESTART_VERSION_IRRIGATION, "the irrigation", "elmk_irrigation_enable", [](Ctx c) { return c->irr_rows ? 2 : 0; },
     [](Ctx c, int i) { return RstRows{ELMK_IRR_RATE + i, 1, c->irr_rows + (size_t)(ELMK_IRR_RATE + i) * (size_t)c->ld}; }},
    {ELMK_RESTART_ROUTING, ELMK_RESTART_VERSION_ROUTING, "the routing state", "elmk_routing_enable with ELMK_OPT_RESTART_CELLS on",
     [](Ctx c) {
       int ids[ROUTE_STATE_MAX];
       return route_state_rows(c, ids);
     },
     [](Ctx c, int i) {
       int ids[ROUTE_STATE_MAX];
       const char* why = nullptr;
       (void)route_state_rows(c, ids);
       return RstRows{ids[i], 1, const_cast<double*>(route_row(c, ids[i], &why))};
     },
     true},
    {ELMK_RESTART_IRRSUP, ELMK_RESTART_VERSION_ROUTING, "the river supply limit's UNMET_SUM", "elmk_irrigation_supply_enable with ELMK_OPT_RESTART_CELLS on",
     [](Ctx c) { return c->restart_cells && c->route.mem && c->irrsup_rows ? 1 : 0; },
     [](Ctx c, int) { return RstRows{ELMK_IRRSUP_UNMET_SUM, 1, c->irrsup_rows + (size_t)ELMK_IRRSUP_UNMET_SUM * (size_t)c->route.cld}; }, true, false}};
constexpr uint32_t RST_MAX_VERSION = RST_V_HEAT;
static_assert(ELMK_HYD_WA == ELMK_HYD_ZWT + 1 && ELMK_IRR_NLEFT == ELMK_IRR_RATE + 1, "the two rows of the image");

RstLayout rst_layout(elmk_ctx* ctx, int64_t gcol0)
{
  RstLayout L;
  for (int f = 0; f < ELMK_NUM_FIELDS; f++) {
    if (g_class.c[f] != ELMK_CLASS_PROGNOSTIC && g_class.c[f] != ELMK_CLASS_SURFACE) continue;
    L.sec.push_back(elmk_restart_section{ELMK_RESTART_FIELD, f, g_fields[f].nlev, g_fields[f].dtype, ctx->ncols, 0, 0});
    L.src.push_back(RstSrc{(char*)ctx->fptr[f], ctx->ld, store_dtype(g_fields[f].dtype), gcol0, f == ELMK_FIELD_snl});
  }
  for (size_t i = 0; i < ctx->hist.size(); i++) {
    const elmk_ctx::HistEntry& e = ctx->hist[i];
    // a cell-row entry (elmk_cell_history_add_row): gridded = 2, the routing's cells, its accumulators a GRIDDED section (g = the cell)
    const bool bycell = e.cells || e.cellrow;
    const int64_t ext = e.cellrow ? ctx->route.ncells : e.cells ? ctx->ogrid.map.nrows : ctx->ncols;
    L.ent.push_back(elmk_restart_entry{e.tape, e.field, e.op, e.cellrow ? 2 : e.cells ? 1 : 0, bycell ? ext : 0});
    L.sec.push_back(elmk_restart_section{bycell ? ELMK_RESTART_GRIDDED : ELMK_RESTART_HISTORY, (int32_t)i, e.nlev, ELMK_F64, ext, 0, 0});
    L.src.push_back(RstSrc{(char*)(double*)e.acc, e.cld, ELMK_F64, bycell ? 0 : gcol0, false});
  }
  for (const elmk_ctx::AccumEntry& e : ctx->accum) L.acc.push_back(elmk_restart_accum{e.src, e.kind, e.dst, 0, e.period, 0});
  for (const RstKind& K : RST_OPTIONAL) {
    const int n = K.count(ctx);
    if (n) {
      L.kinds |= 1u << K.kind;
      L.version = std::max(L.version, K.version);
    }
    for (int i = 0; i < n; i++) {
      const RstRows r = K.rows(ctx, i);
      L.sec.push_back(elmk_restart_section{K.kind, r.id, r.nlev, ELMK_F64, K.cells ? ctx->route.ncells : ctx->ncols, 0, 0});
      L.src.push_back(RstSrc{(char*)r.dev, K.cells ? ctx->route.cld : ctx->ld, ELMK_F64, K.cells ? 0 : gcol0, false});
    }
  }
  if ((L.kinds & (1u << ELMK_RESTART_ROUTING)) && ctx->route.dam.mem) L.version = std::max(L.version, RST_V_RESERVOIR);  // (RES and KRLS)
  if ((L.kinds & (1u << ELMK_RESTART_ROUTING)) && ctx->route.heat.mem) L.version = std::max(L.version, RST_V_HEAT);  // (TT and TR)
  // the accumulator table follows the history entries
  L.header_bytes = align_up(sizeof(elmk_restart_header) + (L.version >= 2 ? 8 : 0) + (L.version >= RST_V_ROUTING ? 8 : 0) + L.acc.size() * sizeof(elmk_restart_accum) +
                                L.ent.size() * sizeof(elmk_restart_entry) + L.sec.size() * sizeof(elmk_restart_section),
                            RST_ALIGN);
  size_t off = L.header_bytes;
  for (elmk_restart_section& s : L.sec) {
    s.offset = off;
    off = align_up(off + (size_t)s.nlev * (size_t)s.extent * elem_size(s.dtype), RST_ALIGN);
  }
  L.total = off;
  return L;
}

// the image cut into chunks of at most RST_CHUNK bytes and RST_MAX_PIECES pieces; chunk k covers image bytes [lo[k], hi[k]) and
// pieces [first[k], first[k + 1]); psec[p] = the section of piece p
struct RstPlan {
  std::vector<RstPiece> pieces;
  std::vector<int> psec;
  std::vector<int> first;
  std::vector<size_t> lo, hi;
  std::vector<int> nbx;
};

RstPlan rst_plan(const RstLayout& L)
{
  RstPlan P;
  size_t start = 0, end = 0;
  int64_t maxn = 0;
  auto close = [&]() {
    P.hi.push_back(end);
    P.nbx.push_back((int)std::min<int64_t>(64, std::max<int64_t>(1, (maxn + 4095) / 4096)));
    maxn = 0;
  };
  for (size_t s = 0; s < L.sec.size(); s++) {
    const elmk_restart_section& S = L.sec[s];
    const RstSrc& R = L.src[s];
    const int es = elem_size(S.dtype);
    const int ses = R.sdtype == ELMK_F32_STORED ? 4 : es;  // bytes of a stored element
    for (int lev = 0; lev < S.nlev; lev++) {
      for (int64_t c = 0; c < S.extent;) {
        const size_t off = S.offset + ((size_t)lev * S.extent + c) * es;
        if (P.first.empty() || off + es > start + RST_CHUNK || (int)P.pieces.size() - P.first.back() >= RST_MAX_PIECES) {
          if (!P.first.empty()) close();
          P.first.push_back((int)P.pieces.size());
          P.lo.push_back(off);
          start = off;
        }
        const int64_t n = std::min<int64_t>(S.extent - c, (int64_t)((start + RST_CHUNK - off) / es));
        P.pieces.push_back(RstPiece{R.dev + ((size_t)lev * R.ld + c) * ses, (int64_t)(off - start), n, R.g0 + c, lev, R.sdtype, S.dtype,
                                    R.snl ? 1 : 0});
        P.psec.push_back((int)s);
        maxn = std::max(maxn, n);
        end = off + (size_t)n * es;
        c += n;
      }
    }
  }
  if (!P.first.empty()) close();
  P.first.push_back((int)P.pieces.size());
  return P;
}

// the call's device and host resources, released on every return path (after the streams are idle)
struct RstCall {
  elmk_ctx* ctx;
  DevBuf<char> stage;
  DevBuf<RstPiece> table;
  DevBuf<uint64_t> part, sums;
  hipStream_t copy = nullptr;
  hipEvent_t packed[2] = {}, copied[2] = {};
  explicit RstCall(elmk_ctx* c) : ctx(c) {}
  ~RstCall()
  {
    (void)hipStreamSynchronize(ctx->stream);
    if (copy) (void)hipStreamSynchronize(copy);
    for (int i = 0; i < 2; i++) {
      if (packed[i]) (void)hipEventDestroy(packed[i]);
      if (copied[i]) (void)hipEventDestroy(copied[i]);
    }
    if (copy) (void)hipStreamDestroy(copy);
  }
  hipError_t alloc(const RstPlan& P, size_t stage_bytes)
  {
    size_t part_n = 0;
    for (size_t k = 0; k + 1 < P.first.size(); k++) part_n = std::max(part_n, (size_t)(P.first[k + 1] - P.first[k]) * P.nbx[k]);
    hipError_t e = stage.alloc(std::max<size_t>(stage_bytes, 256));
    if (!e) e = table.alloc(std::max<size_t>(P.pieces.size(), 1) * sizeof(RstPiece));
    if (!e) e = part.alloc(std::max<size_t>(part_n, 1) * 2 * sizeof(uint64_t));
    if (!e) e = sums.alloc(std::max<size_t>(P.pieces.size(), 1) * 2 * sizeof(uint64_t));
    if (!e && !P.pieces.empty())
      e = hipMemcpyAsync(table, P.pieces.data(), P.pieces.size() * sizeof(RstPiece), hipMemcpyHostToDevice, ctx->stream);
    return e;
  }
};

size_t chunk_bytes(const RstPlan& P)
{
  size_t m = 0;
  for (size_t k = 0; k < P.lo.size(); k++) m = std::max(m, P.hi[k] - P.lo[k]);
  return align_up(m, RST_ALIGN);
}

// per-section sums of the piece sums (checksum, out-of-range count)
void section_sums(const RstPlan& P, const std::vector<uint64_t>& sums, size_t nsec, std::vector<uint64_t>& ck, uint64_t* bad)
{
  ck.assign(nsec, 0);
  *bad = 0;
  for (size_t p = 0; p < P.pieces.size(); p++) {
    ck[P.psec[p]] += sums[2 * p];
    *bad += sums[2 * p + 1];
  }
}

int restart_enter(elmk_ctx* ctx, int64_t gcol0, const void* image, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  if (!image || gcol0 < 0) return invalid(ctx, (std::string(who) + ": bad arguments").c_str());
  if (int rc = refuse_capture(ctx, who)) return rc;
  return synced(ctx);  // every elmk_run and accumulate in flight
}
}  // namespace

namespace elmk {
int field_class(int f) { return g_class.c[f]; }
}  // namespace elmk

extern "C" {

int elmk_field_class(int field) { return field_ok(field) ? g_class.c[field] : ELMK_E_INVALID; }

int elmk_restart_size(elmk_ctx* ctx, int64_t* bytes)
{
  if (int rc = enter(ctx)) return rc;
  if (!bytes) return invalid(ctx, "elmk_restart_size: bad arguments");
  *bytes = (int64_t)rst_layout(ctx, 0).total;
  return ELMK_OK;
}

int elmk_restart_save(elmk_ctx* ctx, int64_t gcol0, void* image, int64_t bytes)
{
  if (int rc = restart_enter(ctx, gcol0, image, "elmk_restart_save")) return rc;
  const RstLayout L = rst_layout(ctx, gcol0);
  if (bytes < (int64_t)L.total) return invalid(ctx, "elmk_restart_save: the buffer is smaller than elmk_restart_size");
  const RstPlan P = rst_plan(L);
  unsigned char* out = (unsigned char*)image;
  const size_t cb = chunk_bytes(P);
  RstCall R(ctx);
  HIPCHK(R.alloc(P, 2 * cb));
  HIPCHK(hipStreamCreateWithFlags(&R.copy, hipStreamNonBlocking));
  for (int i = 0; i < 2; i++) {
    HIPCHK(hipEventCreateWithFlags(&R.packed[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&R.copied[i], hipEventDisableTiming));
  }
  // chunk k is packed into staging slot k % 2 on the context's stream and copied on the copy stream straight into the caller's
  // buffer; chunk k + 1 is enqueued before the copy of chunk k, so it is packed while chunk k crosses the link.  (A copy of pageable
  // memory returns when it is done; a bounce through pinned host chunks plus a host memcpy measured 2.8 times slower at 1 M
  // columns, profiles/r10_restart_cost.jsonl.)
  const int nch = (int)P.lo.size();
  auto pack = [&](int k) -> int {
    if (k >= 2) HIPCHK(hipStreamWaitEvent(ctx->stream, R.copied[k % 2], 0));  // slot k % 2 was read by the copy of chunk k - 2
    launch_restart_pieces(0, (RstPiece*)R.table + P.first[k], P.first[k + 1] - P.first[k], P.nbx[k], (char*)R.stage + (size_t)(k % 2) * cb,
                          R.part, (uint64_t*)R.sums + 2 * (size_t)P.first[k], ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(R.packed[k % 2], ctx->stream));
    return ELMK_OK;
  };
  if (nch > 0)
    if (int rc = pack(0)) return rc;
  for (int k = 0; k < nch; k++) {
    if (k + 1 < nch)
      if (int rc = pack(k + 1)) return rc;
    HIPCHK(hipStreamWaitEvent(R.copy, R.packed[k % 2], 0));
    HIPCHK(hipMemcpyAsync(out + P.lo[k], (char*)R.stage + (size_t)(k % 2) * cb, P.hi[k] - P.lo[k], hipMemcpyDeviceToHost, R.copy));
    HIPCHK(hipEventRecord(R.copied[k % 2], R.copy));
  }
  HIPCHK(hipStreamSynchronize(R.copy));
  std::vector<uint64_t> sums(2 * P.pieces.size());
  unsigned long long counts[ELMK_HIST_MAX_TAPES] = {};
  if (!sums.empty()) HIPCHK(hipMemcpyAsync(sums.data(), R.sums, sums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (ctx->hist_table) HIPCHK(hipMemcpyAsync(counts, hist_counts(ctx), sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  unsigned long long nacc[ELMK_ACCUM_MAX_ENTRIES] = {};
  if (!L.acc.empty())
    HIPCHK(hipMemcpyAsync(nacc, accum_counts(ctx), L.acc.size() * sizeof nacc[0], hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<uint64_t> ck;
  uint64_t bad = 0;
  section_sums(P, sums, L.sec.size(), ck, &bad);
  // the header, the tables and the zero padding after every section
  memset(out, 0, L.header_bytes);
  for (const elmk_restart_section& s : L.sec) {
    const size_t end = s.offset + (size_t)s.nlev * (size_t)s.extent * elem_size(s.dtype);
    memset(out + end, 0, align_up(end, RST_ALIGN) - end);
  }
  elmk_restart_header H{};
  memcpy(H.magic, ELMK_RESTART_MAGIC, 8);
  H.version = L.version;
  H.real_bytes = (uint32_t)store_size(ELMK_F64);
  H.schema_hash = schema_hash();
  H.gcol0 = gcol0;
  H.ncols = ctx->ncols;
  for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++) H.tape_count[t] = counts[t];
  H.nentries = (uint32_t)L.ent.size();
  H.nsections = (uint32_t)L.sec.size();
  H.header_bytes = L.header_bytes;
  H.total_bytes = L.total;
  memcpy(out, &H, sizeof H);
  unsigned char* p = out + sizeof H;
  if (L.version >= 2) {
    const uint32_t word[2] = {(uint32_t)L.acc.size(), 0u};
    memcpy(p, word, 8);
    p += 8;
  }
  if (L.version >= RST_V_ROUTING) {  // the routing's call count
    const int64_t ncalls = ctx->route.ncalls;
    memcpy(p, &ncalls, 8);
    p += 8;
  }
  if (!L.ent.empty()) memcpy(p, L.ent.data(), L.ent.size() * sizeof(elmk_restart_entry));
  p += L.ent.size() * sizeof(elmk_restart_entry);
  for (size_t i = 0; i < L.acc.size(); i++) {
    elmk_restart_accum A = L.acc[i];
    A.nsteps = nacc[i];
    memcpy(p, &A, sizeof A);
    p += sizeof A;
  }
  for (size_t s = 0; s < L.sec.size(); s++) {
    elmk_restart_section S = L.sec[s];
    S.checksum = ck[s];
    memcpy(p + s * sizeof S, &S, sizeof S);
  }
  H.header_checksum = header_checksum(out, L.header_bytes);
  memcpy(out + offsetof(elmk_restart_header, header_checksum), &H.header_checksum, 8);
  return ELMK_OK;
}

int elmk_restart_load(elmk_ctx* ctx, int64_t gcol0, const void* image, int64_t bytes)
{
  if (int rc = restart_enter(ctx, gcol0, image, "elmk_restart_load")) return rc;
  const unsigned char* in = (const unsigned char*)image;
  elmk_restart_header H;
  if (bytes < (int64_t)sizeof H) return invalid(ctx, "elmk_restart_load: truncated image");
  memcpy(&H, in, sizeof H);
  if (memcmp(H.magic, ELMK_RESTART_MAGIC, 8) != 0 || H.version < 1 || H.version > RST_MAX_VERSION)
    return invalid(ctx, "elmk_restart_load: not a restart image of this format version");
  if (H.header_bytes > (uint64_t)bytes || H.total_bytes > (uint64_t)bytes || H.header_bytes % 8 != 0)
    return invalid(ctx, "elmk_restart_load: truncated image");
  if (header_checksum(in, H.header_bytes) != H.header_checksum) return invalid(ctx, "elmk_restart_load: header checksum mismatch");
  if (H.schema_hash != schema_hash()) return invalid(ctx, "elmk_restart_load: the image was saved with another field schema");
  if (H.ncols != ctx->ncols) return invalid(ctx, "elmk_restart_load: the image holds another number of columns");
  if (H.gcol0 != gcol0) return invalid(ctx, "elmk_restart_load: the image starts at another global column");
  const RstLayout L = rst_layout(ctx, gcol0);
  // the optional kinds the image holds: the kind its version stands for, accumulator entries when its count word counts any, and from
  // version 4 on whatever its section table lists; they must be the context's
  const unsigned char* p = in + sizeof H;
  unsigned long long nacc[ELMK_ACCUM_MAX_ENTRIES] = {};
  const char* const acc_differs = "elmk_restart_load: the image's accumulator entries differ from the context's";
  const char* const truncated = "elmk_restart_load: truncated image";
  uint32_t word[2] = {0u, 0u};
  if (H.version >= 2) {
    if (H.header_bytes < sizeof H + 8) return invalid(ctx, truncated);
    memcpy(word, p, 8);
    p += 8;
  }
  int64_t route_ncalls = 0;
  if (H.version >= RST_V_ROUTING) {
    if (H.header_bytes < sizeof H + 16) return invalid(ctx, truncated);
    memcpy(&route_ncalls, p, 8);
    p += 8;
    if (route_ncalls < 0) return invalid(ctx, "elmk_restart_load: the routing's call count is negative");
  }
  unsigned kinds = word[0] ? 1u << ELMK_RESTART_ACCUM : 0u;
  for (const RstKind& K : RST_OPTIONAL) kinds |= K.implied && K.version == H.version ? 1u << K.kind : 0u;
  // (version 7 is version 6 with the reservoirs' two sections, version 8 version 6 with the stream temperature's two)
  if (H.version == RST_V_RESERVOIR || H.version == RST_V_HEAT) kinds |= 1u << ELMK_RESTART_ROUTING;
  std::vector<std::pair<int32_t, int64_t>> img_cells, ctx_cells;  // (id, extent) of the cell sections of the routing state
  if (H.version >= ELMK_RESTART_VERSION_HYDROLOGY) {
    const uint64_t at = (uint64_t)(p - in) + (uint64_t)H.nentries * sizeof(elmk_restart_entry) + (uint64_t)word[0] * sizeof(elmk_restart_accum);
    if (at > H.header_bytes || (H.header_bytes - at) / sizeof(elmk_restart_section) < H.nsections) return invalid(ctx, truncated);
    for (uint32_t k = 0; k < H.nsections; k++) {
      elmk_restart_section S;
      memcpy(&S, in + at + (size_t)k * sizeof S, sizeof S);
      for (const RstKind& K : RST_OPTIONAL) kinds |= K.kind == S.kind ? 1u << K.kind : 0u;
      if (S.kind == ELMK_RESTART_ROUTING) img_cells.emplace_back(S.id, S.extent);
    }
  }
  for (const RstKind& K : RST_OPTIONAL) {
    if (!((kinds ^ L.kinds) & (1u << K.kind))) continue;
    char msg[200];
    if (kinds & (1u << K.kind))
      snprintf(msg, sizeof msg, "elmk_restart_load: the version-%u image holds %s, not enabled in the context (%s)", H.version, K.feature, K.enable);
    else
      snprintf(msg, sizeof msg, "elmk_restart_load: the context has %s (%s) and the version-%u image holds no such rows", K.feature, K.enable, H.version);
    return invalid(ctx, msg);
  }
  if (word[0] != L.acc.size() || word[1] != 0u) return invalid(ctx, acc_differs);
  for (const elmk_restart_section& S : L.sec)
    if (S.kind == ELMK_RESTART_ROUTING) ctx_cells.emplace_back(S.id, S.extent);
  if (img_cells != ctx_cells)
    return invalid(ctx, "elmk_restart_load: the image's routing state differs from the context's: another ncells (elmk_routing_enable), or the "
                        "kinematic-wave scheme (elmk_routing_kinematic_enable), the floodplain inundation (elmk_routing_inundation_enable) or "
                        "the reservoirs (elmk_routing_reservoir_enable) or the stream temperature (elmk_routing_heat_enable) on in one and off in the other");
  // a differing entry table; the feature is named where the image holds an entry over a feature row (ELMK_RESTART_ROW_FIELD, include/
  // elmk_restart.def) that the context has not got in that place
  const auto entries_differ = [&]() {
    const uint64_t room = (H.header_bytes - (uint64_t)(p - in)) / sizeof(elmk_restart_entry);
    for (uint64_t i = 0; i < std::min<uint64_t>(H.nentries, room); i++) {
      elmk_restart_entry E;
      memcpy(&E, p + i * sizeof E, sizeof E);
      if (E.field >= ELMK_RESTART_ROW_BASE && (i >= L.ent.size() || L.ent[i].field != E.field))
        return invalid(ctx, "elmk_restart_load: the image holds history entries over feature rows (elmk_column_history_add_row, elmk_gridded_history_add_row) "
                            "and the context's entries differ from them");
    }
    return invalid(ctx, "elmk_restart_load: the image's history entries differ from the context's");
  };
  if (H.nentries != L.ent.size() || H.nsections != L.sec.size() || H.header_bytes != L.header_bytes || H.total_bytes != L.total)
    return entries_differ();
  for (size_t i = 0; i < L.ent.size(); i++) {
    elmk_restart_entry E;
    memcpy(&E, p + i * sizeof E, sizeof E);
    if (memcmp(&E, &L.ent[i], sizeof E) != 0) return entries_differ();
  }
  p += L.ent.size() * sizeof(elmk_restart_entry);
  for (size_t i = 0; i < L.acc.size(); i++) {
    elmk_restart_accum A;
    memcpy(&A, p, sizeof A);
    p += sizeof A;
    nacc[i] = A.nsteps;
    A.nsteps = 0;  // (loaded, not compared)
    if (memcmp(&A, &L.acc[i], sizeof A) != 0) return invalid(ctx, acc_differs);
  }
  std::vector<uint64_t> want(L.sec.size());
  for (size_t s = 0; s < L.sec.size(); s++) {
    elmk_restart_section S;
    memcpy(&S, p + s * sizeof S, sizeof S);
    want[s] = S.checksum;
    S.checksum = 0;
    if (memcmp(&S, &L.sec[s], sizeof S) != 0) return invalid(ctx, "elmk_restart_load: the image's section table differs from the context's");
  }
  const RstPlan P = rst_plan(L);
  const size_t cb = chunk_bytes(P);
  RstCall R(ctx);
  HIPCHK(R.alloc(P, cb));
  // pass 1: every checksum and the snl range, state untouched; pass 2: scatter into the state and the accumulators
  const int nch = (int)P.lo.size();
  auto pass = [&](int mode) -> int {
    for (int k = 0; k < nch; k++) {
      HIPCHK(hipMemcpyAsync(R.stage, in + P.lo[k], P.hi[k] - P.lo[k], hipMemcpyHostToDevice, ctx->stream));
      launch_restart_pieces(mode, (RstPiece*)R.table + P.first[k], P.first[k + 1] - P.first[k], P.nbx[k], R.stage, R.part,
                            mode == 1 ? (uint64_t*)R.sums + 2 * (size_t)P.first[k] : nullptr, ctx->stream);
      HIPCHK(hipGetLastError());
    }
    return ELMK_OK;
  };
  if (int rc = pass(1)) return rc;
  std::vector<uint64_t> sums(2 * P.pieces.size());
  if (!sums.empty()) HIPCHK(hipMemcpyAsync(sums.data(), R.sums, sums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<uint64_t> ck;
  uint64_t bad = 0;
  section_sums(P, sums, L.sec.size(), ck, &bad);
  for (size_t s = 0; s < L.sec.size(); s++)
    if (ck[s] != want[s]) return invalid(ctx, "elmk_restart_load: section checksum mismatch");
  if (bad) return invalid(ctx, "elmk_restart_load: snl outside 0..nlevsno");
  if (L.kinds & (1u << ELMK_RESTART_ROUTING)) {  // every row of the river stages zero, as their _init calls leave the diagnostic ones
    if (int rc = route_zero_rows(ctx)) return rc;
    if (ctx->irrsup_rows) HIPCHK(hipMemsetAsync(ctx->irrsup_rows, 0, ctx->irrsup_rows.bytes(), ctx->stream));
    ctx->route.ncalls = route_ncalls;
  }
  if (int rc = pass(2)) return rc;  // then the tape counts
  if (ctx->hist_table) {
    unsigned long long counts[ELMK_HIST_MAX_TAPES];
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++) counts[t] = H.tape_count[t];
    HIPCHK(hipMemcpyAsync(hist_counts(ctx), counts, sizeof counts, hipMemcpyHostToDevice, ctx->stream));
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++) ctx->hist_dirty[t] = counts[t] > 0;
  }
  if (!L.acc.empty())
    HIPCHK(hipMemcpyAsync(accum_counts(ctx), nacc, L.acc.size() * sizeof nacc[0], hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

}  // extern "C"
