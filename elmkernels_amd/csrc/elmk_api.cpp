// elmk_api.cpp - host side of the C ABI declared in include/elmk.h.
//
// Owns the device arena (every field of elmk_fields.def as SoA [lev][column], level stride padded to 64
// columns, each field 256-byte aligned), the parameter block (DevState) mirrored into device memory, one
// HIP stream, and a staging buffer for layout conversion.  No physics lives here and there is no CPU path:
// every elmk_<physics>() is a single kernel launch on the context's stream.
#include "elmk.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_maps.h"

using namespace elmk;

namespace {

struct FieldDesc {
  const char* name;
  int dtype;
  int nlev;
};

const FieldDesc g_fields[ELMK_NUM_FIELDS] = {
#define ELMK_FIELD(name, T, nlev) {#name, ELMK_##T, nlev},
#include "elmk_fields.def"
#undef ELMK_FIELD
    {"err_flags", ELMK_U32, 1},
};

inline int elem_size(int dtype) { return dtype == ELMK_F64 ? 8 : (dtype == ELMK_U8 ? 1 : 4); }
// bytes of one element as it is STORED on the device: the report-only ELMK_STATE_F32 build (libelmk_f32.so, BASELINE config 5)
// keeps every fp64 state field as fp32 (elmk_dev.h: field_of); the C ABI still speaks double
#ifdef ELMK_STATE_F32
constexpr bool kStateF32 = true;
#else
constexpr bool kStateF32 = false;
#endif
inline int store_size(int dtype) { return (kStateF32 && dtype == ELMK_F64) ? 4 : elem_size(dtype); }
inline int store_dtype(int dtype) { return (kStateF32 && dtype == ELMK_F64) ? ELMK_F32_STORED : dtype; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

thread_local std::string g_create_error;
constexpr int MAXLEV_STAGE = 21;  // widest field (zisoi)

// The owner of one device allocation (hipMalloc), or with Pinned of one pinned host allocation (hipHostMalloc), and of its size:
// freed by reset() and by its destructor (a move assignment hands the old block to the moved-from owner).  bytes() is what alloc()
// was asked for and 0 while nothing is held, so elmk_device_bytes adds up owners and no release path keeps a count.  Whoever frees
// has synchronised every stream that may still use the memory (hipFree also synchronises the device, but nothing here relies on that).
template <class T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    std::swap(p_, o.p_);
    std::swap(bytes_, o.bytes_);
    return *this;
  }
  ~DevBuf() { (void)reset(); }
  hipError_t alloc(size_t bytes)
  {
    (void)reset();
    void* v = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&v, bytes, hipHostMallocDefault) : hipMalloc(&v, bytes);
    if (e == hipSuccess) {
      p_ = (T*)v;
      bytes_ = bytes;
    }
    return e;
  }
  hipError_t reset()
  {
    const hipError_t e = !p_ ? hipSuccess : Pinned ? hipHostFree(p_) : hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
    return e;
  }
  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

// Lays regions out one after another in one block, each on a 256-byte boundary.  carve() runs a layout twice: over no block to
// size it, then over the allocated block to hand each region's address to its pointer (block.bytes() is the layout's size).
struct Carve {
  char* base;
  size_t bytes = 0;
  template <class P>
  void take(P& dst, size_t n)
  {
    if (base) dst = (P)(base + bytes);
    bytes += align_up(n, 256);
  }
};
template <class Layout>
hipError_t carve(DevBuf<char>& block, Layout layout)
{
  Carve sizing{nullptr};
  layout(sizing);
  if (const hipError_t e = block.alloc(sizing.bytes)) return e;
  Carve place{block};
  layout(place);
  return hipSuccess;
}

// The two map shapes of elmk_maps.h as they lie on the device, inside their owner's block: take() lays the arrays out, upload()
// fills them from the caller's (checked) arrays and returns once the copies are done - the sources are pageable host memory.
struct EllMap {
  int64_t ncells = 0;
  int npts = 0, npad = 0;  // (npad 0: no map)
  int32_t* idx = nullptr;  // [npad][ld]; padding rows and the columns past ncols hold -1
  double* w = nullptr;     // [npad][ld]
  void take(Carve& L, int64_t ncells_, int npts_, size_t ld)
  {
    *this = EllMap{ncells_, npts_, ell_npad(npts_)};
    L.take(idx, (size_t)npad * ld * sizeof(int32_t));
    L.take(w, (size_t)npad * ld * sizeof(double));
  }
  // `what` names the owner in the text of a HIP error; zeroes from w to `end` (the owner's regions behind the map, or the block's end)
  int upload(elmk_ctx* ctx, const char* what, const char* end, const int32_t* hidx, const double* hw) const;
};
struct CsrMap {
  int64_t nrows = 0, nnz = 0;
  int64_t* ptr = nullptr;  // [nrows + 1]
  int32_t* col = nullptr;  // [nnz]
  double* w = nullptr;     // [nnz]
  void take(Carve& L, int64_t nrows_, int64_t nnz_)
  {
    *this = CsrMap{nrows_, nnz_};
    L.take(ptr, (size_t)(nrows + 1) * sizeof(int64_t));
    L.take(col, (size_t)nnz * sizeof(int32_t));
    L.take(w, (size_t)nnz * sizeof(double));
  }
  // after_ptr(): the owner's further copies, enqueued behind ptr's; true if one failed
  template <class More>
  int upload(elmk_ctx* ctx, const int64_t* hptr, const int32_t* hcol, const double* hw, More after_ptr) const;
};

// the list counters of the compacted kernels (ELMK_LIST_COUNT / ELMK_LIST_HEAD, one per CPAD words) and the classes of canopy_fluxes
constexpr size_t COUNTERS_BYTES = ((size_t)(2 * NLISTS + CF_NCLS) * CPAD * 4 + 255) / 256 * 256;

// the captured launch sequences of elmk_set_graph
enum GraphId { GRAPH_TS7, GRAPH_FUSED, GRAPH_ADVANCE, GRAPH_RUN_STEP, GRAPH_N };

}  // namespace

struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  double dt = 0.0;
  hipStream_t stream = nullptr;
  uint64_t tag = 0;  // what else the captured launches depend on (elmk_run: its flags and the history and accumulator tables' versions)
  uint64_t tag2 = 0;  // more of the same (elmk_run: whether the soil hydrology stage is in the step: its flag and the land unit)
  void drop()  // (nothing may still run it)
  {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
  }
};

struct elmk_ctx {
  int dev = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  SideStreams side{};
  int64_t ncols = 0;
  int64_t ld = 0;
  DevState h;            // host mirror of the device parameter block
  DevBuf<DevState> d;    // device copy handed to kernels
  bool dirty = true;
  // every device allocation of the context is one of these DevBuf owners
  DevBuf<char> arena;
  void* fptr[ELMK_NUM_FIELDS] = {};
  DevBuf<double> snicar;
  DevBuf<double> snowage;  // SnwRdsTable (elmk_set_snow_age_tables)
  DevBuf<char> scratch;  // work arrays + work lists + queue counters of the compacted kernels
  // in scratch after DevState::cons_diag (diag [8][ld]): the stage-1 partials [8][ELMK_CONS_NPART][3] and the (min, max, sum)
  // triples [8][3] of launch_conservation
  double* cons_part = nullptr;
  double* cons_out = nullptr;
  DevBuf<char> staging;  // device staging for layout conversion
  std::vector<int> snap_fields;  // elmk_snapshot_fields
  std::vector<DevBuf<double>> snap_bufs;
  DevBuf<uint32_t> red_or;  // device scalars for elmk_error_summary
  long long* red_first = nullptr;
  // elmk_set_graph: the seven wrappers of elmk_timestep7 captured once as a HIP graph (kernel nodes + the side-stream
  // fork / join of albedo_snicar) and replayed; key = (dt, stream)
  bool use_graph = false;
  bool have_init_params = false;
  GraphSlot graph[GRAPH_N];
  // A HIP error may have cut a step short between the kernel that fills a work list and the one that drains it and leaves it
  // empty (the lists have no reset launch of their own): the next physics call zeroes every list counter first.
  bool lists_stale = false;
  // per-column solar geometry: DevState::geo and DevState::col_dayl in one allocation (elmk_set_column_geography); the mode flag
  // itself is side.col_dayl (elmk_solar_geometry sets it, elmk_clear_column_geography clears it)
  DevBuf<double> geo;
  bool geo_set = false;
  // history (elmk_history_*): the entries, their rows as the device table k_hist_accumulate reads (hist_table: the column rows, one
  // count per tape, then the cell rows of gridded entries), and per tape whether it has accumulated since its last reset
  // (elmk_history_add refuses such a tape).  A gridded entry (elmk_gridded_history_add) has cell rows: nlev x cld accumulators over
  // the output grid's cells, cld = ncells rounded up to 64; their bytes are counted in elmk_device_bytes.
  struct HistEntry {
    int tape, field, op, nlev, row0;
    DevBuf<double> acc;
    bool cells = false;
    int64_t cld = 0;
  };
  std::vector<HistEntry> hist;
  std::vector<HistRow> hist_rows;
  std::vector<HistRow> hist_crows;
  DevBuf<HistRow> hist_table;
  bool hist_dirty[ELMK_HIST_MAX_TAPES] = {};
  uint64_t hist_version = 0;  // counts elmk_history_add / _clear: a captured step of elmk_run holds the table of its moment
  // accumulated fields (elmk_accum_*): the entries, their rows as the device table k_accum_update reads (accum_table: the rows, then
  // one step count per entry); elmk_device_bytes counts the table and every value buffer
  struct AccumEntry {
    int src, kind, dst, nlev, row0;
    int64_t period;
    DevBuf<double> val;
  };
  std::vector<AccumEntry> accum;
  std::vector<AccumRow> accum_rows;
  DevBuf<char> accum_table;
  uint64_t accum_version = 0;  // counts elmk_accum_add / _clear, as hist_version
  // active layer thickness (elmk_active_layer_*): the rows alt, altmax, altmax_lastyear [3][ld] in fp64, held exactly while the feature
  // is enabled
  DevBuf<double> alt_rows;
  // soil hydrology (elmk_soil_hydrology_*): the ELMK_HYD_NROWS fp64 rows [row][ld], held exactly while the feature is enabled
  DevBuf<double> hyd_rows;
  bool hyd_params = false;  // elmk_soil_hydrology_set_params has been called since the enable
  bool snowage_set = false;
  // multi-step runs (elmk_run_reserve, elmk_series_upload, elmk_run): one device allocation `mem` holds the forcing series, the
  // phenology series, the two step tables, the step cursor and the two diagnostics rings (buffer b: rows b * max_steps ..); `rows`
  // is the pinned host copy of the step tables.  Per buffer, what the run last enqueued on it reads and the event of its end
  // (run_done): a buffer is reused only after that run has finished, so the read set of every unfinished run is known to
  // elmk_series_upload.  A new reservation starts from Run{}.
  struct Run {
    int slots = 0, max_steps = 0;
    int64_t fcols = 0, fstride = 0;  // forcing series: entries per record (columns, or cells in grid mode) and the record stride
    DevBuf<char> mem;
    char* forc = nullptr;
    char* phen = nullptr;
    RunRow* table = nullptr;
    int32_t* cursor = nullptr;
    double* cons = nullptr;
    uint32_t* flag_or = nullptr;
    long long* flag_first = nullptr;
    DevBuf<RunRow, true> rows;
    bool live[2] = {};
    int slot_lo[2] = {}, slot_hi[2] = {};
    unsigned months[2] = {};
    unsigned aer_months[2] = {};  // the months of the aerosol series the run reads (ELMK_RUN_AEROSOL; 0 without the flag)
    uint64_t count = 0;  // runs enqueued since the reserve
    int last_buf = -1, last_nsteps = 0;
    int flags = 0;  // of the run being enqueued (the run step's stages)
    // shortwave COSZEN mode (elmk_series_record_times): the record-time scalars of every forcing slot (elmk_solar_step_consts at
    // forc_dt and the slot's record start), allocated by the first call after a reservation, and which slots have one
    DevBuf<elmk_solar_step> rec;
    std::vector<char> rec_set;
  } run;
  hipStream_t upload = nullptr;  // of elmk_series_upload, with run_done created by the first elmk_run_reserve
  hipEvent_t run_done[2] = {};
  // forcing on a coarser grid (elmk_set_forcing_grid): one allocation `mem` holds the ELL map and the fp64 staging of
  // elmk_upload_gridded (map.ncells values)
  struct Grid {
    DevBuf<char> mem;
    EllMap map;
    double* cells = nullptr;
  } grid;
  // output grid (elmk_set_output_grid): one allocation `mem` holds the CSR map by output cell (map.nrows cells)
  struct OGrid {
    double fill = 0.0;
    DevBuf<char> mem;
    CsrMap map;
  } ogrid;
  // shortwave (elmk_set_shortwave_mode): the mode, the forcing records' interval, and in COSZEN mode czf - every column's mean
  // cos(zenith) over the current forcing record's interval ([ld] doubles, allocated when the context first enters COSZEN mode).
  // step_time: elmk_set_forcing_record_time has written czf for elmk_get_forcing (an elmk_run overwrites it); czf_ready: czf holds the
  // values of the last record time or run step (elmk_download_forcing_cosz)
  struct Shortwave {
    int mode = ELMK_SW_REFERENCE;
    double forc_dt = 0.0;
    DevBuf<double> czf;
    bool step_time = false, czf_ready = false;
  } sw;
  // downscaling (elmk_set_downscaling): the mode and its parameters; topo = the elevations [2][ld] (row 0 the columns', row 1 the
  // forcing's surface height), allocated by the first call that sets either, and which rows hold values.  Longwave groups
  // (elmk_set_downscaling_groups): one allocation `gmem` holds the CSR map by group, each group's weight sum wsum (the host's sum in
  // term order) and the Lg row [ld] the TOPO forcing kernels write for launch_ds_lw_norm.
  struct Downscale {
    int mode = ELMK_DS_OFF;
    double lapse = 0.006, lapse_lw = 0.032, lw_limit = 0.5;
    DevBuf<double> topo;
    bool col_set = false, forc_set = false;
    DevBuf<char> gmem;
    CsrMap groups;
    double* wsum = nullptr;
    double* lg = nullptr;
  } ds;
  // aerosol deposition (elmk_aerosol_reserve): one allocation `mem` holds the cell series [AER_NSTREAM][12][map.ncells] in fp64 and, unless
  // the series is per column (map.npad 0), the ELL map of its grid.  step_live: a
  // stepwise elmk_aerosol_deposition has been enqueued since the last elmk_aerosol_upload waited for aer_step_done.
  struct Aerosol {
    DevBuf<char> mem;
    double* cells = nullptr;
    EllMap map;  // (per-column series: only its ncells, = ncols)
    bool step_live = false;
  } aer;
  hipEvent_t aer_step_done = nullptr;  // the end of the last stepwise elmk_aerosol_deposition (created by the first reservation)
  std::string err;
};

namespace {

bool hip_fail(elmk_ctx* ctx, hipError_t e, const char* what)
{
  if (e == hipSuccess) return false;
  char buf[512];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  if (ctx) {
    ctx->err = buf;
    ctx->lists_stale = true;
  }
  g_create_error = buf;
  return true;
}

#define HIPCHK(call)                                      \
  do {                                                    \
    if (hip_fail(ctx, (call), #call)) return ELMK_E_HIP;  \
  } while (0)

// Owner of the events of the diagnostic entry points: released on every return path
struct EventList {
  std::vector<hipEvent_t> ev;
  hipError_t create(size_t n)
  {
    ev.reserve(n);
    for (size_t i = 0; i < n; i++) {
      hipEvent_t e = nullptr;
      const hipError_t rc = hipEventCreate(&e);
      if (rc != hipSuccess) return rc;
      ev.push_back(e);
    }
    return hipSuccess;
  }
  hipEvent_t& operator[](size_t i) { return ev[i]; }
  ~EventList()
  {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

int invalid(elmk_ctx* ctx, const char* msg)
{
  if (ctx) ctx->err = msg;
  g_create_error = msg;
  return ELMK_E_INVALID;
}

int EllMap::upload(elmk_ctx* ctx, const char* what, const char* end, const int32_t* hidx, const double* hw) const
{
  const std::string set = std::string("hipMemset(") + what, copy = std::string("hipMemcpy2D(") + what;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  // padding rows and the columns past ncols: idx -1 (all bits set), w 0; then the caller's npts rows
  if (npad && (hip_fail(ctx, hipMemsetAsync(idx, 0xFF, (char*)w - (char*)idx, ctx->stream), (set + " idx)").c_str()) ||
               hip_fail(ctx, hipMemsetAsync(w, 0, end - (char*)w, ctx->stream), (set + " w)").c_str())))
    return ELMK_E_HIP;
  if (npad && n > 0 &&
      (hip_fail(ctx, hipMemcpy2DAsync(idx, ld * sizeof(int32_t), hidx, n * sizeof(int32_t), n * sizeof(int32_t), (size_t)npts,
                                      hipMemcpyHostToDevice, ctx->stream), (copy + " idx)").c_str()) ||
       hip_fail(ctx, hipMemcpy2DAsync(w, ld * sizeof(double), hw, n * sizeof(double), n * sizeof(double), (size_t)npts,
                                      hipMemcpyHostToDevice, ctx->stream), (copy + " w)").c_str())))
    return ELMK_E_HIP;
  return hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize") ? ELMK_E_HIP : ELMK_OK;
}

template <class More>
int CsrMap::upload(elmk_ctx* ctx, const int64_t* hptr, const int32_t* hcol, const double* hw, More after_ptr) const
{
  const bool failed =
      hip_fail(ctx, hipMemcpyAsync(ptr, hptr, (size_t)(nrows + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(ptr)") ||
      after_ptr() ||
      (nnz > 0 && (hip_fail(ctx, hipMemcpyAsync(col, hcol, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(col)") ||
                   hip_fail(ctx, hipMemcpyAsync(w, hw, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(w)"))) ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
  return failed ? ELMK_E_HIP : ELMK_OK;
}

// a refusal of elmk_maps.h's checks (text, or nullptr for none) under the entry point's name
int invalid_map(elmk_ctx* ctx, const char* who, const char* text)
{
  return text ? invalid(ctx, (std::string(who) + ": " + text).c_str()) : ELMK_OK;
}

int push_params(elmk_ctx* ctx)
{
  if (!ctx->dirty) return ELMK_OK;
  HIPCHK(hipMemcpyAsync(ctx->d, &ctx->h, sizeof(DevState), hipMemcpyHostToDevice, ctx->stream));
  // the source is pageable host memory: the runtime has staged it before returning, so h may change again
  ctx->dirty = false;
  return ELMK_OK;
}

int enter(elmk_ctx* ctx)
{
  if (!ctx) return ELMK_E_INVALID;
  HIPCHK(hipSetDevice(ctx->dev));
  return ELMK_OK;
}

// wait for the runs in flight (they read the series, maps, elevations and tables the caller is about to change) and, with `uploads`,
// for the copy stream (it may still write them), then drop the captured run step (it holds their addresses and the kernels of their
// modes and widths)
int quiesce(elmk_ctx* ctx, bool uploads)
{
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (uploads && ctx->upload) HIPCHK(hipStreamSynchronize(ctx->upload));
  ctx->graph[GRAPH_RUN_STEP].drop();
  return ELMK_OK;
}

// never write under a run that reads it: wait for the end of every enqueued, unfinished run whose buffer b `reads` selects
template <class Pred>
int wait_for_runs(elmk_ctx* ctx, Pred reads)
{
  for (int b = 0; b < 2; b++)
    if (ctx->run.live[b] && reads(b)) HIPCHK(hipEventSynchronize(ctx->run_done[b]));
  return ELMK_OK;
}

bool field_ok(int f) { return f >= 0 && f < ELMK_NUM_FIELDS; }
int field_class(int f);  // include/elmk_restart.def (defined with the restart images)

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------
// lifetime
// ---------------------------------------------------------------------------------------------------
int elmk_create(int64_t ncols, int device_id, elmk_ctx** out)
{
  if (!out || ncols < 0) return invalid(nullptr, "elmk_create: bad arguments");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = std::string("elmk_create: no HIP device (") + hipGetErrorString(e) +
                     "); libelmk has no CPU fallback";
    return ELMK_E_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= ndev) {
    g_create_error = "elmk_create: device id out of range";
    return ELMK_E_NO_DEVICE;
  }
  elmk_ctx* ctx = new (std::nothrow) elmk_ctx();
  if (!ctx) return ELMK_E_NOMEM;
  ctx->dev = device_id;
  ctx->ncols = ncols;
  ctx->ld = (int64_t)align_up((size_t)(ncols > 0 ? ncols : 1), 64);

  auto fail = [&](int code) {
    elmk_destroy(ctx);
    return code;
  };
  if (hip_fail(ctx, hipSetDevice(device_id), "hipSetDevice")) return fail(ELMK_E_HIP);
  if (hip_fail(ctx, hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking), "hipStreamCreate"))
    return fail(ELMK_E_HIP);
  ctx->stream = ctx->own_stream;
  for (int i = 0; i < ELMK_NSIDE; i++) {
    if (hip_fail(ctx, hipStreamCreateWithFlags(&ctx->side.s[i], hipStreamNonBlocking), "hipStreamCreate(side)") ||
        hip_fail(ctx, hipEventCreateWithFlags(&ctx->side.join[i], hipEventDisableTiming), "hipEventCreate"))
      return fail(ELMK_E_HIP);
  }
  if (hip_fail(ctx, hipEventCreateWithFlags(&ctx->side.fork, hipEventDisableTiming), "hipEventCreate")) return fail(ELMK_E_HIP);

  // parameter block defaults: LandType() (land_data.h:38) and ELMState scalars (elm_state.h:221-224); the allocations below set
  // its device pointers
  DevState& h = ctx->h;
  memset(&h, 0, sizeof h);
  h.ncols = ncols;
  h.ld = ctx->ld;
  h.land = Land{1, 0, 2, 0, 0};
  h.dewmx = 0.1;
  h.oldfflag = 1;

  const size_t ld = (size_t)ctx->ld;
  if (hip_fail(ctx, carve(ctx->arena, [&](Carve& L) {
                 for (int f = 0; f < ELMK_NUM_FIELDS; f++) L.take(ctx->fptr[f], (size_t)g_fields[f].nlev * ld * store_size(g_fields[f].dtype));
               }), "hipMalloc(state arena)"))
    return fail(ELMK_E_NOMEM);
  if (hip_fail(ctx, hipMemsetAsync(ctx->arena, 0, ctx->arena.bytes(), ctx->stream), "hipMemset(state arena)")) return fail(ELMK_E_HIP);

  if (hip_fail(ctx, ctx->snicar.alloc(SN_TOTAL * sizeof(double)), "hipMalloc(snicar)")) return fail(ELMK_E_NOMEM);
  if (hip_fail(ctx, hipMemsetAsync(ctx->snicar, 0, SN_TOTAL * sizeof(double), ctx->stream), "hipMemset(snicar)"))
    return fail(ELMK_E_HIP);
  if (hip_fail(ctx, ctx->snowage.alloc(3 * ELMK_SNOWAGE_N * sizeof(double)), "hipMalloc(snowage)")) return fail(ELMK_E_NOMEM);
  if (hip_fail(ctx, hipMemsetAsync(ctx->snowage, 0, 3 * ELMK_SNOWAGE_N * sizeof(double), ctx->stream), "hipMemset(snowage)"))
    return fail(ELMK_E_HIP);
  if (hip_fail(ctx, ctx->d.alloc(sizeof(DevState)), "hipMalloc(params)")) return fail(ELMK_E_NOMEM);
  // canopy_fluxes queue records (k_canopy_fluxes.hip), by queue position
  const int64_t cf_nblk = (ncols + 255) / 256 > 0 ? (ncols + 255) / 256 : 1;
  h.cf_nblk = cf_nblk;
  if (hip_fail(ctx, carve(ctx->scratch, [&](Carve& L) {
                 L.take(h.wk, (size_t)WK_N * ld * 8);
                 L.take(h.lists, (size_t)NLISTS * ld * 4);
                 L.take(h.counters, COUNTERS_BYTES);
                 L.take(h.cf_niter, ld * 4);
                 L.take(h.cf_rec, (size_t)CF_REC_N * (ld + 8) * 8);
                 L.take(h.cf_fin, (size_t)CF_FIN_N * (ld + 8) * 8);
                 L.take(h.cf_irec, (size_t)CF_IREC_N * ld * 4);
                 L.take(h.cf_pos, ld * 4);
                 L.take(h.cf_blk, (size_t)CF_NCLS * (size_t)cf_nblk * 4);
                 L.take(h.cf_cls, ld);
                 L.take(h.cf_given, 3 * ld * 8);
                 L.take(h.alb_snow, 28 * ld * 8);
                 L.take(h.cons_diag, 8 * ld * 8);
                 L.take(ctx->cons_part, (size_t)8 * ELMK_CONS_NPART * 3 * 8);
                 L.take(ctx->cons_out, 8 * 3 * 8);
               }), "hipMalloc(scratch)"))
    return fail(ELMK_E_NOMEM);
  if (hip_fail(ctx, hipMemsetAsync(ctx->scratch, 0, ctx->scratch.bytes(), ctx->stream), "hipMemset(scratch)"))
    return fail(ELMK_E_HIP);
  if (hip_fail(ctx, ctx->red_or.alloc(16), "hipMalloc(reduce)")) return fail(ELMK_E_NOMEM);
  ctx->red_first = (long long*)(ctx->red_or + 2);

  // staging: up to 32 MiB, at least one 64-column tile of the widest field
  size_t want = (size_t)MAXLEV_STAGE * 8 * (size_t)(ncols > 0 ? ncols : 1);
  if (want > ((size_t)32 << 20)) want = (size_t)32 << 20;
  if (want < (size_t)MAXLEV_STAGE * 8 * 64) want = (size_t)MAXLEV_STAGE * 8 * 64;
  if (hip_fail(ctx, ctx->staging.alloc(want), "hipMalloc(staging)")) return fail(ELMK_E_NOMEM);

  h.snicar = (gptr<const double>)(double*)ctx->snicar;
  h.snowage = (gptr<const double>)(double*)ctx->snowage;
  {
    int f = 0;
#define ELMK_FIELD(name, T, nlev) h.name = field_of<ELMK_##T>::from(ctx->fptr[f++]);
#include "elmk_fields.def"
#undef ELMK_FIELD
    h.err_flags = (gptr<uint32_t>)ctx->fptr[f];
  }
  ctx->dirty = true;
  if (hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) return fail(ELMK_E_HIP);
  *out = ctx;
  return ELMK_OK;
}

int elmk_destroy(elmk_ctx* ctx)
{
  if (!ctx) return ELMK_OK;
  (void)hipSetDevice(ctx->dev);
  // 1. nothing may still use the context's memory: its stream (the caller's, once set), the side streams and the upload stream
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (hipStream_t s : ctx->side.s)
    if (s) (void)hipStreamSynchronize(s);
  if (ctx->upload) (void)hipStreamSynchronize(ctx->upload);
  // 2. the graph executables
  for (GraphSlot& g : ctx->graph) g.drop();
  // 3. the memory: every allocation is a DevBuf member of the context
  const SideStreams side = ctx->side;
  const hipStream_t own = ctx->own_stream, upload = ctx->upload;
  const hipEvent_t done[3] = {ctx->run_done[0], ctx->run_done[1], ctx->aer_step_done};
  delete ctx;
  // 4. the events and streams
  for (int i = 0; i < ELMK_NSIDE; i++) {
    if (side.s[i]) (void)hipStreamDestroy(side.s[i]);
    if (side.join[i]) (void)hipEventDestroy(side.join[i]);
  }
  if (side.fork) (void)hipEventDestroy(side.fork);
  for (hipEvent_t e : done)
    if (e) (void)hipEventDestroy(e);
  if (upload) (void)hipStreamDestroy(upload);
  if (own) (void)hipStreamDestroy(own);
  return ELMK_OK;
}

const char* elmk_last_error(const elmk_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int elmk_set_stream(elmk_ctx* ctx, void* hip_stream)
{
  if (int rc = enter(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return ELMK_OK;
}

namespace {
// a captured graph holds the launch shape and the kernels of the moment it was captured (elmk_set_option, the day-length mode)
int drop_graphs(elmk_ctx* ctx)
{
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (GraphSlot& g : ctx->graph) g.drop();
  return ELMK_OK;
}

// per-column day length on or off (DevState::col_dayl, elmk_kernels.h: SideStreams::col_dayl)
int set_col_dayl(elmk_ctx* ctx, bool on)
{
  if (ctx->side.col_dayl == on) return ELMK_OK;
  if (int rc = drop_graphs(ctx)) return rc;
  ctx->side.col_dayl = on;
  return ELMK_OK;
}

// the calls that allocate, free or wait cannot be part of a caller's captured graph
int refuse_capture(elmk_ctx* ctx, const char* msg)
{
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hip_fail(ctx, hipStreamIsCapturing(ctx->stream, &cap), "hipStreamIsCapturing")) return ELMK_E_HIP;
  return cap != hipStreamCaptureStatusNone ? invalid(ctx, msg) : ELMK_OK;
}
}  // namespace

int elmk_set_graph(elmk_ctx* ctx, int on)
{
  if (int rc = enter(ctx)) return rc;
  ctx->use_graph = on != 0;
  return ctx->use_graph ? ELMK_OK : drop_graphs(ctx);
}

int elmk_set_option(elmk_ctx* ctx, int option, int value)
{
  if (int rc = enter(ctx)) return rc;
  if (option == ELMK_OPT_ALB_STAGED) {
    const bool want = value != 0;
    if (want != ctx->side.alb_staged) {
      if (int rc = drop_graphs(ctx)) return rc;  // (a captured graph holds the kernels of the structure it was captured in)
      ctx->side.alb_staged = want;
    }
    return ELMK_OK;
  }
  if (option != ELMK_OPT_CF_HALF_WORKGROUPS) return invalid(ctx, "elmk_set_option: unknown option");
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->dev));
  const int want = value ? (cus > 0 ? cus : 256) : 0;
  if (want != ctx->side.cf_half_groups) {
    if (int rc = drop_graphs(ctx)) return rc;
    ctx->side.cf_half_groups = want;
  }
  return ELMK_OK;
}

int elmk_sync(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int64_t elmk_ncols(const elmk_ctx* ctx) { return ctx ? ctx->ncols : -1; }
int64_t elmk_level_stride(const elmk_ctx* ctx) { return ctx ? ctx->ld : -1; }
int64_t elmk_device_bytes(const elmk_ctx* ctx)
{
  if (!ctx) return -1;
  size_t n = ctx->arena.bytes() + ctx->staging.bytes() + ctx->scratch.bytes() + ctx->snicar.bytes() + ctx->snowage.bytes() + ctx->d.bytes() +
             ctx->run.mem.bytes() + ctx->grid.mem.bytes() + ctx->ogrid.mem.bytes() + ctx->sw.czf.bytes() + ctx->run.rec.bytes() +
             ctx->ds.topo.bytes() + ctx->ds.gmem.bytes() + ctx->accum_table.bytes() + ctx->aer.mem.bytes() + ctx->alt_rows.bytes() +
             ctx->hyd_rows.bytes();
  // the cell rows of gridded history entries (not the column rows) and the accumulators' values: whole rows of ld or cld doubles,
  // both multiples of 64, so every size is a multiple of 256 already
  for (const elmk_ctx::HistEntry& e : ctx->hist) n += e.cells ? e.acc.bytes() : 0;
  for (const elmk_ctx::AccumEntry& e : ctx->accum) n += e.val.bytes();
  return (int64_t)n;
}

// ---------------------------------------------------------------------------------------------------
// schema
// ---------------------------------------------------------------------------------------------------
int elmk_num_fields(void) { return ELMK_NUM_FIELDS; }
const char* elmk_field_name(int field) { return field_ok(field) ? g_fields[field].name : nullptr; }
int elmk_field_id(const char* name)
{
  if (!name) return -1;
  for (int f = 0; f < ELMK_NUM_FIELDS; f++)
    if (strcmp(name, g_fields[f].name) == 0) return f;
  return -1;
}
int elmk_field_info(int field, int* nlev, int* dtype)
{
  if (!field_ok(field)) return ELMK_E_INVALID;
  if (nlev) *nlev = g_fields[field].nlev;
  if (dtype) *dtype = g_fields[field].dtype;
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// data movement
// ---------------------------------------------------------------------------------------------------
// Columns [col0, col0 + n) of nlev device rows, ld elements of es bytes apart, from (up) or to the host's n > 0 columns: as rows of n
// elements (ELMK_LAYOUT_SOA, or one level), else in the reference layout [col][lev] through the device staging buffer in chunks of
// whole 64-column tiles.  Enqueued on the context's stream, which is waited for only where a chunk reuses the staging buffer: the
// caller waits for the end (the host side is pageable memory).
static int xfer_rows(elmk_ctx* ctx, char* dev, int64_t ld, int es, int nlev, void* host, int64_t col0, int64_t n, int layout, bool up)
{
  if (layout == ELMK_LAYOUT_SOA || nlev == 1) {
    if (up)
      HIPCHK(hipMemcpy2DAsync(dev + (size_t)col0 * es, (size_t)ld * es, host, (size_t)n * es, (size_t)n * es, nlev, hipMemcpyHostToDevice,
                              ctx->stream));
    else
      HIPCHK(hipMemcpy2DAsync(host, (size_t)n * es, dev + (size_t)col0 * es, (size_t)ld * es, (size_t)n * es, nlev, hipMemcpyDeviceToHost,
                              ctx->stream));
    return ELMK_OK;
  }
  const int64_t chunk = (int64_t)(ctx->staging.bytes() / ((size_t)nlev * es)) / 64 * 64;
  if (chunk <= 0) return invalid(ctx, "staging buffer too small");
  for (int64_t done = 0; done < n; done += chunk) {
    if (done > 0) HIPCHK(hipStreamSynchronize(ctx->stream));  // staging is reused by this chunk
    const int64_t m = (n - done) < chunk ? (n - done) : chunk;
    char* hp = (char*)host + (size_t)done * nlev * es;
    if (up) {
      HIPCHK(hipMemcpyAsync(ctx->staging, hp, (size_t)m * nlev * es, hipMemcpyHostToDevice, ctx->stream));
      launch_cols_to_soa(ctx->staging, dev, es, nlev, ld, col0 + done, m, ctx->stream);
    } else {
      launch_soa_to_cols(dev, ctx->staging, es, nlev, ld, col0 + done, m, ctx->stream);
      HIPCHK(hipMemcpyAsync(hp, ctx->staging, (size_t)m * nlev * es, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipGetLastError());
  }
  return ELMK_OK;
}

// host elements already in the stored element type
static int xfer_stored(elmk_ctx* ctx, int field, void* host, int64_t col0, int64_t n, int layout, bool up)
{
  const int nlev = g_fields[field].nlev;
  if (layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR && nlev != 1) return invalid(ctx, "elmk_upload/download: unknown layout");
  if (int rc = xfer_rows(ctx, (char*)ctx->fptr[field], ctx->ld, store_size(g_fields[field].dtype), nlev, host, col0, n, layout, up)) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

static int xfer(elmk_ctx* ctx, int field, void* host, int64_t col0, int64_t n, int layout, bool up)
{
  if (int rc = enter(ctx)) return rc;
  if (!field_ok(field) || (!host && n > 0) || col0 < 0 || n < 0 || col0 + n > ctx->ncols)
    return invalid(ctx, "elmk_upload/download: bad field or column range");
  if (n == 0) return ELMK_OK;
  // snl indexes the level arrays (top = nlevsno - snl) in every snow and soil kernel, in global memory and in LDS packs: a
  // value outside 0..nlevsno is refused at the two doors host values come through (here and elmk_fill) instead of being read
  // out of bounds on the device (the reference has the same undefined behaviour, but no such door)
  if (up && field == ELMK_FIELD_snl) {
    const int32_t* v = (const int32_t*)host;
    for (int64_t i = 0; i < n; i++)
      if (v[i] < 0 || v[i] > NLEVSNO) return invalid(ctx, "elmk_upload: snl outside 0..nlevsno");
  }
  if (kStateF32 && g_fields[field].dtype == ELMK_F64) {
    // fp32-state build: the caller's doubles are rounded to the stored fp32 on the way in and widened on the way out (on the
    // host: this build is a measurement variant, its benchmark tiles a small uploaded block on the device)
    const size_t cnt = (size_t)n * (size_t)g_fields[field].nlev;
    std::vector<float> tmp(cnt);
    double* h = (double*)host;
    if (up)
      for (size_t i = 0; i < cnt; i++) tmp[i] = (float)h[i];
    const int rc = xfer_stored(ctx, field, tmp.data(), col0, n, layout, up);
    if (rc == ELMK_OK && !up)
      for (size_t i = 0; i < cnt; i++) h[i] = (double)tmp[i];
    return rc;
  }
  return xfer_stored(ctx, field, host, col0, n, layout, up);
}

int elmk_upload(elmk_ctx* ctx, int field, const void* host, int64_t col0, int64_t n, int layout)
{
  return xfer(ctx, field, const_cast<void*>(host), col0, n, layout, true);
}
int elmk_download(elmk_ctx* ctx, int field, void* host, int64_t col0, int64_t n, int layout)
{
  return xfer(ctx, field, host, col0, n, layout, false);
}

int elmk_fill(elmk_ctx* ctx, int field, double value)
{
  if (int rc = enter(ctx)) return rc;
  if (!field_ok(field)) return invalid(ctx, "elmk_fill: bad field");
  if (field == ELMK_FIELD_snl && !(value >= 0.0 && value <= (double)NLEVSNO))
    return invalid(ctx, "elmk_fill: snl outside 0..nlevsno");
  launch_fill(ctx->fptr[field], store_dtype(g_fields[field].dtype), g_fields[field].nlev, ctx->ld, ctx->ncols, value, ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

void* elmk_device_ptr(elmk_ctx* ctx, int field) { return (ctx && field_ok(field)) ? ctx->fptr[field] : nullptr; }

int elmk_tile_columns(elmk_ctx* ctx, int64_t nbase, uint64_t seed, int nrules, const elmk_perturb* rules)
{
  if (int rc = enter(ctx)) return rc;
  if (nbase <= 0 || nbase > ctx->ncols || nrules < 0 || (nrules > 0 && !rules))
    return invalid(ctx, "elmk_tile_columns: bad arguments");
  for (int f = 0; f < ELMK_NUM_FIELDS; f++) {
    int mode = -1;
    double amp = 0.0;
    for (int r = 0; r < nrules; r++) {
      if (rules[r].field == f) {
        mode = rules[r].mode;
        amp = rules[r].amp;
      }
    }
    launch_tile(ctx->fptr[f], store_dtype(g_fields[f].dtype), g_fields[f].nlev, ctx->ld, ctx->ncols, nbase, seed, f, mode, amp,
                ctx->stream);
  }
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_snapshot_fields(elmk_ctx* ctx, const int* fields, int nfields)
{
  if (int rc = enter(ctx)) return rc;
  if (nfields < 0 || (nfields > 0 && !fields)) return invalid(ctx, "elmk_snapshot_fields: bad arguments");
  for (int i = 0; i < nfields; i++)
    if (!field_ok(fields[i])) return invalid(ctx, "elmk_snapshot_fields: unknown field");
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->snap_bufs.clear();
  ctx->snap_fields.clear();
  // a field enters the snapshot only once its buffer exists and its copy has been enqueued; any failure drops the whole
  // snapshot, so that a later elmk_restore_fields never restores from a partly filled set
  int rc = ELMK_OK;
  for (int i = 0; i < nfields && rc == ELMK_OK; i++) {
    const int f = fields[i];
    const size_t bytes = (size_t)g_fields[f].nlev * (size_t)ctx->ld * store_size(g_fields[f].dtype);
    DevBuf<double> b;
    if (hip_fail(ctx, b.alloc(bytes), "hipMalloc(snapshot)"))
      rc = ELMK_E_NOMEM;
    else if (hip_fail(ctx, hipMemcpyAsync(b, ctx->fptr[f], bytes, hipMemcpyDeviceToDevice, ctx->stream), "hipMemcpyAsync(snapshot)"))
      rc = ELMK_E_HIP;
    else {
      ctx->snap_bufs.push_back(std::move(b));
      ctx->snap_fields.push_back(f);
    }
  }
  if (rc == ELMK_OK && hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(snapshot)")) rc = ELMK_E_HIP;
  if (rc != ELMK_OK) {
    (void)hipStreamSynchronize(ctx->stream);
    ctx->snap_bufs.clear();
    ctx->snap_fields.clear();
  }
  return rc;
}

int elmk_restore_fields(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  // plain streaming kernels (hipMemcpyAsync device-to-device goes through the SDMA engines here, ~80 GB/s), up to
  // COPY_JOBS_MAX fields per launch: a small field's copy is all launch latency
  CopyJobs J;
  J.n = 0;
  int64_t words = 0;
  for (size_t i = 0; i < ctx->snap_fields.size(); i++) {
    const int f = ctx->snap_fields[i];
    const size_t bytes = (size_t)g_fields[f].nlev * (size_t)ctx->ld * store_size(g_fields[f].dtype);
    words += (int64_t)(bytes / 8);
    J.src[J.n] = ctx->snap_bufs[i];
    J.dst[J.n] = (double*)ctx->fptr[f];
    J.end[J.n] = words;
    J.n++;
    if (J.n == COPY_JOBS_MAX || i + 1 == ctx->snap_fields.size()) {
      launch_copy_multi(J, ctx->stream);
      J.n = 0;
      words = 0;
    }
  }
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------------------
int elmk_set_land(elmk_ctx* ctx, int ltype, int ctype, int vtype, int urbpoi, int lakpoi)
{
  if (!ctx) return ELMK_E_INVALID;
  if (vtype < 0 || vtype >= ELMK_MXPFT) return invalid(ctx, "elmk_set_land: vtype out of range");
  ctx->h.land = Land{ltype, ctype, vtype, urbpoi != 0, lakpoi != 0};
  ctx->dirty = true;
  return ELMK_OK;
}

int elmk_set_scalars(elmk_ctx* ctx, double dewmx, int oldfflag, double dayl, double max_dayl)
{
  if (!ctx) return ELMK_E_INVALID;
  ctx->h.dewmx = dewmx;
  ctx->h.oldfflag = oldfflag;
  ctx->h.dayl = dayl;
  ctx->h.max_dayl = max_dayl;
  ctx->dirty = true;
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// per-column solar geometry (elmk_solar.h, k_solar.hip)
// ---------------------------------------------------------------------------------------------------
int elmk_set_column_geography(elmk_ctx* ctx, const double* lat_r, const double* lon_r)
{
  if (int rc = enter(ctx)) return rc;
  if (!lat_r || !lon_r) return invalid(ctx, "elmk_set_column_geography: null pointer");
  const int64_t ld = ctx->ld;
  // the time-invariant terms of every column, with the host libm (the reference's bits by construction)
  std::vector<double> g((size_t)ELMK_GEO_N * (size_t)ld, 0.0);
  for (int64_t c = 0; c < ctx->ncols; c++) {
    if (!elmk_solar_geography_ok(lat_r[c], lon_r[c])) {
      char buf[200];
      snprintf(buf, sizeof buf, "elmk_set_column_geography: column %lld: lat %g / lon %g (need |lat| <= pi/2 + 10 eps, finite lon)",
               (long long)c, lat_r[c], lon_r[c]);
      return invalid(ctx, buf);
    }
    double row[ELMK_GEO_N];
    elmk_solar_column_consts(lat_r[c], lon_r[c], row);
    for (int k = 0; k < ELMK_GEO_N; k++) g[(size_t)k * ld + c] = row[k];
  }
  if (!ctx->geo) {
    const size_t bytes = (size_t)(ELMK_GEO_N + COL_DAYL_N) * (size_t)ld * 8;
    HIPCHK(ctx->geo.alloc(bytes));
    HIPCHK(hipMemsetAsync(ctx->geo, 0, bytes, ctx->stream));
    ctx->h.geo = (gptr<const double>)(double*)ctx->geo;
    ctx->h.col_dayl = (gptr<double>)(ctx->geo + (size_t)ELMK_GEO_N * ld);
    ctx->dirty = true;
  }
  HIPCHK(hipMemcpyAsync(ctx->geo, g.data(), g.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));  // (g goes out of scope)
  ctx->geo_set = true;
  return ELMK_OK;
}

int elmk_solar_geometry(elmk_ctx* ctx, double dt_seconds, double decday, int doy)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->geo_set) return invalid(ctx, "elmk_solar_geometry: no column geography (elmk_set_column_geography)");
  if (!(dt_seconds > 0.0 && dt_seconds <= 1.0e9) || !(decday >= 0.0 && decday < 1.0e9) || doy < -1 || doy > 1000000000)
    return invalid(ctx, "elmk_solar_geometry: bad dt / decday / doy");
  // canopy_fluxes switches to the per-column kernels: graphs captured so far hold the scalar ones
  if (int rc = set_col_dayl(ctx, true)) return rc;
  if (int rc = push_params(ctx)) return rc;
  launch_solar_geometry(ctx->d, ctx->ncols, elmk_solar_step_consts(dt_seconds, decday, doy), ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_download_day_length(elmk_ctx* ctx, double* dayl, double* max_dayl)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->side.col_dayl) return invalid(ctx, "elmk_download_day_length: no elmk_solar_geometry since the geography was set");
  const size_t bytes = (size_t)ctx->ncols * 8;
  if (dayl && bytes)
    HIPCHK(hipMemcpyAsync(dayl, ctx->geo + (size_t)(ELMK_GEO_N + COL_DAYL) * ctx->ld, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (max_dayl && bytes)
    HIPCHK(hipMemcpyAsync(max_dayl, ctx->geo + (size_t)ELMK_GEO_MAX_DAYL * ctx->ld, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

namespace {
int sw_reset(elmk_ctx* ctx, int mode, double forc_dt);
}

int elmk_clear_column_geography(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = set_col_dayl(ctx, false)) return rc;
  if (ctx->sw.mode != ELMK_SW_REFERENCE)  // COSZEN needs the geography
    if (int rc = sw_reset(ctx, ELMK_SW_REFERENCE, 0.0)) return rc;
  if (ctx->geo) {
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const hipError_t e = ctx->geo.reset();
    ctx->h.geo = nullptr;
    ctx->h.col_dayl = nullptr;
    ctx->dirty = true;
    HIPCHK(e);
  }
  ctx->geo_set = false;
  return ELMK_OK;
}

int elmk_set_pft(elmk_ctx* ctx, const double* psn, const double* alb, const double* z0mr, const double* displar)
{
  if (!ctx || !psn || !alb || !z0mr || !displar) return invalid(ctx, "elmk_set_pft: null table");
  memcpy(ctx->h.pft_psn, psn, sizeof ctx->h.pft_psn);
  memcpy(ctx->h.pft_alb, alb, sizeof ctx->h.pft_alb);
  memcpy(ctx->h.z0mr, z0mr, sizeof ctx->h.z0mr);
  memcpy(ctx->h.displar, displar, sizeof ctx->h.displar);
  ctx->dirty = true;
  return ELMK_OK;
}

int elmk_set_init_params(elmk_ctx* ctx, double organic_max, const double* roota_par, const double* rootb_par)
{
  if (!ctx || !roota_par || !rootb_par) return invalid(ctx, "elmk_set_init_params: null table");
  if (!(organic_max > 0.0)) return invalid(ctx, "elmk_set_init_params: organic_max must be positive");
  ctx->h.organic_max = organic_max;
  memcpy(ctx->h.roota_par, roota_par, sizeof ctx->h.roota_par);
  memcpy(ctx->h.rootb_par, rootb_par, sizeof ctx->h.rootb_par);
  ctx->dirty = true;
  ctx->have_init_params = true;
  return ELMK_OK;
}

int elmk_set_soilcolor(elmk_ctx* ctx, const double* albsat, const double* albdry)
{
  if (!ctx || !albsat || !albdry) return invalid(ctx, "elmk_set_soilcolor: null table");
  memcpy(ctx->h.albsat, albsat, sizeof ctx->h.albsat);
  memcpy(ctx->h.albdry, albdry, sizeof ctx->h.albdry);
  ctx->dirty = true;
  return ELMK_OK;
}

int elmk_set_snicar(elmk_ctx* ctx, const elmk_snicar_tables* t)
{
  if (int rc = enter(ctx)) return rc;
  if (!t) return invalid(ctx, "elmk_set_snicar: null");
  std::vector<double> buf(SN_TOTAL, 0.0);
  const double* aer[6][3] = {
      {t->ss_alb_oc1, t->asm_prm_oc1, t->ext_cff_mss_oc1},    {t->ss_alb_oc2, t->asm_prm_oc2, t->ext_cff_mss_oc2},
      {t->ss_alb_dst1, t->asm_prm_dst1, t->ext_cff_mss_dst1}, {t->ss_alb_dst2, t->asm_prm_dst2, t->ext_cff_mss_dst2},
      {t->ss_alb_dst3, t->asm_prm_dst3, t->ext_cff_mss_dst3}, {t->ss_alb_dst4, t->asm_prm_dst4, t->ext_cff_mss_dst4}};
  for (int s = 0; s < 6; s++)
    for (int p = 0; p < 3; p++) {
      if (!aer[s][p]) return invalid(ctx, "elmk_set_snicar: null aerosol table");
      memcpy(&buf[SN_OC1 + s * SN_AER_STRIDE + p * 5], aer[s][p], 5 * sizeof(double));
    }
  const double* snw[2][3] = {{t->ss_alb_snw_drc, t->asm_prm_snw_drc, t->ext_cff_mss_snw_drc},
                             {t->ss_alb_snw_dfs, t->asm_prm_snw_dfs, t->ext_cff_mss_snw_dfs}};
  for (int k = 0; k < 2; k++)
    for (int p = 0; p < 3; p++) {
      if (!snw[k][p]) return invalid(ctx, "elmk_set_snicar: null Mie table");
      memcpy(&buf[(k == 0 ? SN_SNW_DRC : SN_SNW_DFS) + p * 5 * ELMK_MIE_N], snw[k][p], 5 * ELMK_MIE_N * sizeof(double));
    }
  const double* bc[2][3] = {{t->ss_alb_bc1, t->asm_prm_bc1, t->ext_cff_mss_bc1},
                            {t->ss_alb_bc2, t->asm_prm_bc2, t->ext_cff_mss_bc2}};
  for (int k = 0; k < 2; k++)
    for (int p = 0; p < 3; p++) {
      if (!bc[k][p]) return invalid(ctx, "elmk_set_snicar: null BC table");
      memcpy(&buf[(k == 0 ? SN_BC1 : SN_BC2) + p * 50], bc[k][p], 50 * sizeof(double));
    }
  if (!t->bcenh) return invalid(ctx, "elmk_set_snicar: null bcenh");
  memcpy(&buf[SN_BCENH], t->bcenh, 400 * sizeof(double));
  HIPCHK(hipMemcpyAsync(ctx->snicar, buf.data(), SN_TOTAL * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_set_snow_age_tables(elmk_ctx* ctx, const double* tau, const double* kappa, const double* drdt0)
{
  if (int rc = enter(ctx)) return rc;
  if (!tau || !kappa || !drdt0) return invalid(ctx, "elmk_set_snow_age_tables: null table");
  const double* src[3] = {tau, kappa, drdt0};
  for (int k = 0; k < 3; k++)
    HIPCHK(hipMemcpyAsync(ctx->snowage + (size_t)k * ELMK_SNOWAGE_N, src[k], ELMK_SNOWAGE_N * sizeof(double), hipMemcpyHostToDevice,
                          ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  ctx->snowage_set = true;
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// history (k_history.hip)
// ---------------------------------------------------------------------------------------------------
namespace {
constexpr int HIST_MAX_ROWS = ELMK_HIST_MAX_ENTRIES * MAXLEV_STAGE;
constexpr size_t HIST_COUNTS_OFF = ((size_t)HIST_MAX_ROWS * sizeof(HistRow) + 255) / 256 * 256;
constexpr size_t HIST_CROWS_OFF = HIST_COUNTS_OFF + 256;  // the cell rows of gridded entries
constexpr size_t HIST_TABLE_BYTES = HIST_CROWS_OFF + (size_t)HIST_MAX_ROWS * sizeof(HistRow);
static_assert(ELMK_HIST_MAX_TAPES * sizeof(unsigned long long) <= 256, "the counts fit before the cell rows");

unsigned long long* hist_counts(elmk_ctx* ctx) { return (unsigned long long*)((char*)(HistRow*)ctx->hist_table + HIST_COUNTS_OFF); }
HistRow* hist_cell_rows(elmk_ctx* ctx) { return (HistRow*)((char*)(HistRow*)ctx->hist_table + HIST_CROWS_OFF); }

OGridMap ogrid_map(const elmk_ctx* ctx)
{
  const CsrMap& M = ctx->ogrid.map;
  return OGridMap{M.ptr, M.col, M.w, M.nrows, ctx->ogrid.fill};
}

bool has_gridded_entries(const elmk_ctx* ctx) { return !ctx->hist_crows.empty(); }

unsigned hist_tape_mask(const elmk_ctx* ctx)
{
  unsigned m = 0;
  for (const elmk_ctx::HistEntry& e : ctx->hist) m |= 1u << e.tape;
  return m;
}

// the tapes of mask hold samples: elmk_history_add refuses them until their reset
void mark_sampled(elmk_ctx* ctx, unsigned mask)
{
  for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++)
    if (mask & (1u << t)) ctx->hist_dirty[t] = true;
}

bool tape_ok(int tape) { return tape >= 0 && tape < ELMK_HIST_MAX_TAPES; }
}  // namespace

}  // extern "C"

namespace {
// elmk_history_add (cells = false: accumulators over the columns) and elmk_gridded_history_add (cells = true: over the output grid's
// cells); `who` names the entry point in the messages
int hist_add(elmk_ctx* ctx, int tape, int field, int op, bool cells, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  const std::string w = who;
  if (!tape_ok(tape)) return invalid(ctx, (w + ": unknown tape").c_str());
  if (!field_ok(field)) return invalid(ctx, (w + ": unknown field").c_str());
  if (op < ELMK_HIST_AVG || op > ELMK_HIST_INST) return invalid(ctx, (w + ": unknown op").c_str());
  if (cells && !ctx->ogrid.mem) return invalid(ctx, (w + ": no output grid (elmk_set_output_grid)").c_str());
  if ((int)ctx->hist.size() >= ELMK_HIST_MAX_ENTRIES) return invalid(ctx, (w + ": the history table is full").c_str());
  if (ctx->hist_dirty[tape]) return invalid(ctx, (w + ": the tape holds samples; reset it first").c_str());
  if (int rc = refuse_capture(ctx, (w + ": the stream is being captured").c_str())) return rc;
  if (!ctx->hist_table) {
    HIPCHK(ctx->hist_table.alloc(HIST_TABLE_BYTES));
    HIPCHK(hipMemsetAsync(ctx->hist_table, 0, HIST_TABLE_BYTES, ctx->stream));
  }
  const int nlev = g_fields[field].nlev;
  // a column row spans the level stride; a cell row the cell count rounded up to 64 (16-byte aligned rows for k_hist_reset's pairs)
  const int64_t ld = cells ? (ctx->ogrid.map.nrows + 63) / 64 * 64 : ctx->ld;
  const size_t bytes = (size_t)nlev * (size_t)ld * sizeof(double);
  DevBuf<double> acc;
  if (hip_fail(ctx, acc.alloc(bytes), "hipMalloc(history)")) return ELMK_E_NOMEM;
  launch_fill(acc, ELMK_F64, nlev, ld, ld, hist_init_value(op), ctx->stream);
  std::vector<HistRow>& rows = cells ? ctx->hist_crows : ctx->hist_rows;
  HistRow* table = cells ? hist_cell_rows(ctx) : (HistRow*)ctx->hist_table;
  const int row0 = (int)rows.size();
  const int es = store_size(g_fields[field].dtype);
  for (int l = 0; l < nlev; l++)
    rows.push_back(HistRow{(const char*)ctx->fptr[field] + (size_t)l * (size_t)ctx->ld * es, acc + (size_t)l * (size_t)ld,
                           store_dtype(g_fields[field].dtype), op, tape, 0});
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
  ctx->hist.push_back(elmk_ctx::HistEntry{tape, field, op, nlev, row0, std::move(acc), cells, ld});
  ctx->hist_version++;
  return (int)ctx->hist.size() - 1;
}

// every row of every tape, one launch: the column rows alone as before any gridded entry existed, else with the cell rows after them
void hist_accumulate_launch(elmk_ctx* ctx)
{
  const unsigned mask = hist_tape_mask(ctx);
  if (!has_gridded_entries(ctx))
    launch_hist_accumulate(ctx->hist_table, (int)ctx->hist_rows.size(), hist_counts(ctx), ctx->ncols, mask, ctx->stream);
  else
    launch_hist_accumulate_cells(ctx->hist_table, (int)ctx->hist_rows.size(), hist_cell_rows(ctx), (int)ctx->hist_crows.size(),
                                 ogrid_map(ctx), hist_counts(ctx), ctx->ncols, mask, ctx->stream);
}
}  // namespace

extern "C" {

int elmk_history_add(elmk_ctx* ctx, int tape, int field, int op) { return hist_add(ctx, tape, field, op, false, "elmk_history_add"); }

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
  const int64_t lim = e.cells ? ctx->ogrid.map.nrows : ctx->ncols;  // a gridded entry's col0, n index cells
  if ((!host && n > 0) || col0 < 0 || n < 0 || col0 + n > lim)
    return invalid(ctx, e.cells ? "elmk_history_read: bad cell range" : "elmk_history_read: bad column range");
  if (layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR) return invalid(ctx, "elmk_history_read: unknown layout");
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
      launch_hist_finalize(e.acc, ctx->ld, e.nlev, e.op, count, col0 + done, m, soa, ctx->stream);
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
  if (ctx->hist_table)
    HIPCHK(hipMemsetAsync(hist_counts(ctx), 0, ELMK_HIST_MAX_TAPES * sizeof(unsigned long long), ctx->stream));
  for (bool& d : ctx->hist_dirty) d = false;
  ctx->hist_version++;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

}  // extern "C" (the launch machinery below has templates)

// ---------------------------------------------------------------------------------------------------
// accumulated fields (k_accum.hip; include/elmk.h "accumulated fields")
// ---------------------------------------------------------------------------------------------------
namespace {
constexpr int ACCUM_MAX_ROWS = ELMK_ACCUM_MAX_ENTRIES * MAXLEV_STAGE;
constexpr size_t ACCUM_COUNTS_OFF = ((size_t)ACCUM_MAX_ROWS * sizeof(AccumRow) + 255) / 256 * 256;
constexpr size_t ACCUM_TABLE_BYTES = ACCUM_COUNTS_OFF + 256;
static_assert(ELMK_ACCUM_MAX_ENTRIES * sizeof(unsigned long long) <= 256, "the counts fit behind the rows");

unsigned long long* accum_counts(elmk_ctx* ctx) { return (unsigned long long*)((char*)ctx->accum_table + ACCUM_COUNTS_OFF); }

// every row of every entry, then the counts (two launches; nothing without entries)
void accum_update_launch(elmk_ctx* ctx)
{
  launch_accum_update((const AccumRow*)(char*)ctx->accum_table, (int)ctx->accum_rows.size(), accum_counts(ctx), (int)ctx->accum.size(),
                      ctx->ncols, ctx->stream);
}
}  // namespace

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
  if (int rc = refuse_capture(ctx, "elmk_accum_add: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_accum_init: the stream is being captured")) return rc;
  if (host) {
    if (ctx->ncols > 0)
      if (int rc = xfer_rows(ctx, (char*)(double*)e.val, ctx->ld, 8, e.nlev, const_cast<double*>(host), 0, ctx->ncols, ELMK_LAYOUT_SOA, true)) return rc;
  } else {
    launch_accum_seed(ctx->fptr[e.dst], store_dtype(ELMK_F64), e.val, e.nlev, ctx->ld, ctx->ncols, ctx->stream);
    HIPCHK(hipGetLastError());
  }
  const unsigned long long n = (unsigned long long)nsteps;
  HIPCHK(hipMemcpyAsync(accum_counts(ctx) + entry, &n, sizeof n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_accum_update(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->accum.empty()) return ELMK_OK;
  accum_update_launch(ctx);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_accum_read(elmk_ctx* ctx, int entry, double* host, int64_t col0, int64_t n, int layout, int64_t* nsteps)
{
  if (int rc = enter(ctx)) return rc;
  if (entry < 0 || entry >= (int)ctx->accum.size()) return invalid(ctx, "elmk_accum_read: unknown entry");
  if ((!host && n > 0) || col0 < 0 || n < 0 || col0 + n > ctx->ncols) return invalid(ctx, "elmk_accum_read: bad column range");
  if (layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR) return invalid(ctx, "elmk_accum_read: unknown layout");
  if (int rc = refuse_capture(ctx, "elmk_accum_read: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_accum_clear: the stream is being captured")) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (ctx->accum.empty()) return ELMK_OK;
  ctx->accum.clear();
  ctx->accum_rows.clear();
  HIPCHK(ctx->accum_table.reset());
  ctx->accum_version++;
  return ELMK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// active layer thickness (k_active_layer.hip; include/elmk.h "active layer thickness")
// ---------------------------------------------------------------------------------------------------
namespace {
ActiveLayerArgs alt_args(const elmk_ctx* ctx)
{
  return ActiveLayerArgs{ctx->fptr[ELMK_FIELD_t_soisno], ctx->fptr[ELMK_FIELD_zsoi], (int32_t*)ctx->fptr[ELMK_FIELD_altmax_indx],
                         (int32_t*)ctx->fptr[ELMK_FIELD_altmax_lastyear_indx], ctx->alt_rows,
                         ctx->geo + (size_t)ELMK_GEO_SIN_LAT * (size_t)ctx->ld, ctx->ld, ctx->ncols};
}
static_assert(ELMK_ALT_ALTMAX_LASTYEAR == 2, "three rows");
constexpr int ALT_NROWS = 3;
}  // namespace

extern "C" {

int elmk_active_layer_enable(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->alt_rows) return invalid(ctx, "elmk_active_layer_enable: already enabled");
  if (int rc = refuse_capture(ctx, "elmk_active_layer_enable: the stream is being captured")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its flags' moment)
  const size_t bytes = (size_t)ALT_NROWS * (size_t)ctx->ld * sizeof(double);
  if (hip_fail(ctx, ctx->alt_rows.alloc(bytes), "hipMalloc(active layer rows)")) return ELMK_E_NOMEM;
  if (hip_fail(ctx, hipMemsetAsync(ctx->alt_rows, 0, bytes, ctx->stream), "hipMemset(active layer rows)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->alt_rows.reset();
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

int elmk_active_layer_init(elmk_ctx* ctx, const double* altmax, const double* altmax_lastyear)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->alt_rows) return invalid(ctx, "elmk_active_layer_init: not enabled (elmk_active_layer_enable)");
  if (int rc = refuse_capture(ctx, "elmk_active_layer_init: the stream is being captured")) return rc;
  const size_t ld = (size_t)ctx->ld, n = (size_t)ctx->ncols;
  HIPCHK(hipMemsetAsync(ctx->alt_rows, 0, ctx->alt_rows.bytes(), ctx->stream));
  if (altmax && n) HIPCHK(hipMemcpyAsync(ctx->alt_rows + ELMK_ALT_ALTMAX * ld, altmax, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (altmax_lastyear && n)
    HIPCHK(hipMemcpyAsync(ctx->alt_rows + ELMK_ALT_ALTMAX_LASTYEAR * ld, altmax_lastyear, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_active_layer_update(elmk_ctx* ctx, int rollover)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->alt_rows) return invalid(ctx, "elmk_active_layer_update: not enabled (elmk_active_layer_enable)");
  if (!ctx->geo_set) return invalid(ctx, "elmk_active_layer_update: no column geography (elmk_set_column_geography)");
  if (rollover & ~(ELMK_ALT_ROLL_NORTH | ELMK_ALT_ROLL_SOUTH)) return invalid(ctx, "elmk_active_layer_update: unknown rollover bits");
  launch_active_layer(alt_args(ctx), rollover, ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_active_layer_read(elmk_ctx* ctx, int which, double* host, int64_t col0, int64_t n)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->alt_rows) return invalid(ctx, "elmk_active_layer_read: not enabled (elmk_active_layer_enable)");
  if (which < ELMK_ALT_ALT || which > ELMK_ALT_ALTMAX_LASTYEAR) return invalid(ctx, "elmk_active_layer_read: unknown row");
  if ((!host && n > 0) || col0 < 0 || n < 0 || col0 + n > ctx->ncols) return invalid(ctx, "elmk_active_layer_read: bad column range");
  if (int rc = refuse_capture(ctx, "elmk_active_layer_read: the stream is being captured")) return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->alt_rows + (size_t)which * (size_t)ctx->ld + (size_t)col0, (size_t)n * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_active_layer_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_active_layer_clear: the stream is being captured")) return rc;
  if (!ctx->alt_rows) return ELMK_OK;
  if (int rc = quiesce(ctx, false)) return rc;
  HIPCHK(ctx->alt_rows.reset());
  return ELMK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// physics wrappers: one launch each, same order/arguments as driver/kokkos
// ---------------------------------------------------------------------------------------------------

namespace {
int heal_lists(elmk_ctx* ctx)
{
  if (!ctx->lists_stale) return ELMK_OK;
  ctx->lists_stale = false;
  HIPCHK(hipMemsetAsync(ELMK_GENERIC(ctx->h.counters), 0, COUNTERS_BYTES, ctx->stream));
  return ELMK_OK;
}

// what every physics entry point does before it launches
int enter_physics(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = heal_lists(ctx)) return rc;
  return push_params(ctx);
}

// roctx ranges named after the labels the reference gives its parallel_for launches (driver/kokkos/*_kokkos.cc:
// "kokkos_canhydro_fracwet_kernel", "kokkos_albedo_and_snicar", ...), so that a marker trace of this library reads like one of
// the reference (tracing).  Off unless ELMK_ROCTX=1 is set when the first context is created; the marker
// library is looked up at run time (no link dependency), and a missing one just leaves the ranges off.
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx()
  {
    const char* e = getenv("ELMK_ROCTX");
    if (!e || e[0] != '1') return;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
      if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (push && pop) return;
        push = nullptr;
        pop = nullptr;
      }
    }
  }
};
const Roctx* roctx()
{
  static const Roctx r;
  return &r;
}
// label nullptr: no range
struct RoctxRange {
  const bool on;
  explicit RoctxRange(const char* label) : on(label && roctx()->push)
  {
    if (on) roctx()->push(label);
  }
  ~RoctxRange()
  {
    if (on) roctx()->pop();
  }
};

// ELMInterface::advance order (elm_kokkos_interface.cc:289-307).  ONE stage list per launch sequence drives the plain path, the
// graph capture, the profiled path and the entry points of a single stage, so that they cannot drift apart.
struct Stage {
  void (*launch)(elmk_ctx* ctx, double dt);
  const char* label;  // of its roctx range (nullptr: none)
};
// consecutive stages of one list
struct Stages {
  const Stage* s;
  int n;
  template <int N>
  constexpr Stages(const Stage (&a)[N]) : s(a), n(N) {}
  constexpr Stages(const Stage& one) : s(&one), n(1) {}
};

void stage_frac_wet(elmk_ctx* ctx, double) { launch_frac_wet(ctx->d, ctx->ncols, ctx->stream); }
void stage_albedo_snicar(elmk_ctx* ctx, double) { launch_albedo_snicar(ctx->d, ctx->ncols, ctx->stream, &ctx->side); }
void stage_canopy_hydrology(elmk_ctx* ctx, double dt) { launch_canopy_hydrology(ctx->d, ctx->ncols, dt, ctx->stream); }
void stage_surface_radiation(elmk_ctx* ctx, double) { launch_surface_radiation(ctx->d, ctx->ncols, ctx->stream); }
void stage_canopy_temperature(elmk_ctx* ctx, double) { launch_canopy_temperature(ctx->d, ctx->ncols, ctx->stream); }
void stage_bareground_fluxes(elmk_ctx* ctx, double) { launch_bareground_fluxes(ctx->d, ctx->ncols, ctx->stream); }
void stage_canopy_fluxes(elmk_ctx* ctx, double dt) { launch_canopy_fluxes(ctx->d, ctx->ncols, dt, ctx->stream, 0, &ctx->side); }
template <int K>
void stage_fused(elmk_ctx* ctx, double dt)
{
  launch_fused_stage(ctx->d, ctx->ncols, dt, ctx->stream, &ctx->side, K);
}
void stage_soil_temperature(elmk_ctx* ctx, double dt) { launch_soil_temperature(ctx->d, ctx->ncols, dt, ctx->stream); }
void stage_snow_hydrology(elmk_ctx* ctx, double dt) { launch_snow_hydrology(ctx->d, ctx->ncols, dt, ctx->stream); }
void stage_surface_fluxes(elmk_ctx* ctx, double dt) { launch_surface_fluxes(ctx->d, ctx->ncols, dt, ctx->stream); }

// elmk_timestep7, in the order of ELMK_WRAPPER_FRAC_WET .. ELMK_WRAPPER_CANOPY_FLUXES
constexpr Stage TS7[] = {{stage_frac_wet, "kokkos_canhydro_fracwet_kernel"},   {stage_albedo_snicar, "kokkos_albedo_and_snicar"},
                         {stage_canopy_hydrology, "kokkos_canopy_hydrology"},   {stage_surface_radiation, "kokkos_surface_radiation"},
                         {stage_canopy_temperature, "kokkos_canopy_temperature"}, {stage_bareground_fluxes, "kokkos_bareground_fluxes"},
                         {stage_canopy_fluxes, "kokkos_canopy_fluxes"}};
// elmk_timestep7_fused: the same seven wrappers as ELMK_FUSED_NSTAGE launch groups (k_canopy_fluxes.hip)
constexpr Stage FUSED[] = {{stage_fused<0>, nullptr}, {stage_fused<1>, nullptr}, {stage_fused<2>, nullptr}, {stage_fused<3>, nullptr},
                           {stage_fused<4>, nullptr}};
static_assert(sizeof FUSED / sizeof FUSED[0] == ELMK_FUSED_NSTAGE, "fused stages");
// elmk_advance_physics: the fused seven, then the rest of ELMInterface::advance's per-column calls in its order
constexpr Stage SOIL_TEMPERATURE{stage_soil_temperature, nullptr}, SNOW_HYDROLOGY{stage_snow_hydrology, nullptr},
    SURFACE_FLUXES{stage_surface_fluxes, nullptr};
constexpr Stage ADVANCE[] = {FUSED[0], FUSED[1], FUSED[2], FUSED[3], FUSED[4], SOIL_TEMPERATURE, SNOW_HYDROLOGY, SURFACE_FLUXES};

void launch(elmk_ctx* ctx, const Stage& st, double dt)
{
  const RoctxRange range(st.label);
  st.launch(ctx, dt);
}

// the stages in order; marks (may be null): events recorded on the context's stream before the first stage and after the last,
// and with per_stage before every stage (marks[k] before stage k)
int enqueue_stages(elmk_ctx* ctx, Stages L, double dt, hipEvent_t* marks = nullptr, bool per_stage = true)
{
  for (int k = 0; k < L.n; k++) {
    if (marks && (per_stage || k == 0)) HIPCHK(hipEventRecord(marks[k], ctx->stream));
    launch(ctx, L.s[k], dt);
  }
  if (marks) HIPCHK(hipEventRecord(marks[per_stage ? L.n : 1], ctx->stream));
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

// the stages captured once as a HIP graph (kernel nodes in one chain: the side-stream forks are issued in order on the
// capturing stream) and replayed
int run_graph(elmk_ctx* ctx, GraphSlot& g, Stages L, double dt, uint64_t tag, uint64_t tag2)
{
  if (!g.exec || g.dt != dt || g.stream != ctx->stream || g.tag != tag || g.tag2 != tag2) {
    if (g.exec) {
      // dt or the stream changed: the old executable may still be running its last launch.  (Best effort: a caller that
      // destroyed the old stream has synchronised it itself, and the error of waiting on it is not this call's.)
      if (g.stream && hipStreamSynchronize(g.stream) != hipSuccess) (void)hipGetLastError();
      g.drop();
    }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->side.one_stream = true;  // one chain of nodes: no fork onto the side streams (elmk_kernels.h: SideStreams)
    for (int k = 0; k < L.n; k++) launch(ctx, L.s[k], dt);
    ctx->side.one_stream = false;
    // a launch that failed during capture leaves its error in the runtime and may have invalidated the capture: read it,
    // and ALWAYS end the capture so that neither the stream nor the forked side streams stay in capture mode
    const hipError_t launch_err = hipGetLastError();
    const hipError_t end_err = hipStreamEndCapture(ctx->stream, &graph);
    if (launch_err != hipSuccess || end_err != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      hip_fail(ctx, launch_err != hipSuccess ? launch_err : end_err,
               launch_err != hipSuccess ? "kernel launch during graph capture" : "hipStreamEndCapture");
      return ELMK_E_HIP;
    }
    const hipError_t e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (hip_fail(ctx, e, "hipGraphInstantiate")) {
      g.exec = nullptr;
      return ELMK_E_HIP;
    }
    g.dt = dt;
    g.stream = ctx->stream;
    g.tag = tag;
    g.tag2 = tag2;
  }
  HIPCHK(hipGraphLaunch(g.exec, ctx->stream));
  return ELMK_OK;
}

// a sequence elmk_set_graph applies to: replayed from its captured graph, or enqueued stage by stage
int launch_sequence(elmk_ctx* ctx, GraphId id, Stages L, double dt, uint64_t tag = 0, uint64_t tag2 = 0)
{
  if (ctx->use_graph) return run_graph(ctx, ctx->graph[id], L, dt, tag, tag2);
  return enqueue_stages(ctx, L, dt);
}

// the entry points of one stage
int launch_stage(elmk_ctx* ctx, const Stage& st, double dt)
{
  if (int rc = enter_physics(ctx)) return rc;
  return enqueue_stages(ctx, st, dt);
}

// nsteps profiled steps: HIP events around each step and, with per_stage, between its stages, on the context's stream
// (step_label: a roctx range around each step); the snapshot (if any) is restored before every step outside the event
// brackets, so each profiled step does the same work as the caller's timed loop
int profile_stages(elmk_ctx* ctx, Stages L, double dt, int nsteps, bool per_stage, const char* step_label, float* ms_per_stage,
                   float* ms_total, float* ms_each_step)
{
  const int nev = per_stage ? L.n + 1 : 2;  // events per step
  EventList ev;
  HIPCHK(ev.create((size_t)nsteps * nev));
  for (int s = 0; s < nsteps; s++) {
    if (!ctx->snap_fields.empty())
      if (int rc = elmk_restore_fields(ctx)) return rc;
    const RoctxRange range(step_label);
    if (int rc = enqueue_stages(ctx, L, dt, &ev[(size_t)s * nev], per_stage)) return rc;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<double> acc((size_t)L.n, 0.0);
  double tot = 0.0;
  for (int s = 0; s < nsteps; s++) {
    hipEvent_t* e = &ev[(size_t)s * nev];
    for (int k = 0; per_stage && k < L.n; k++) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, e[k], e[k + 1]));
      acc[k] += ms;
    }
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e[0], e[nev - 1]));
    tot += ms;
    if (ms_each_step) ms_each_step[s] = ms;
  }
  if (ms_per_stage)
    for (int k = 0; k < L.n; k++) ms_per_stage[k] = (float)(acc[k] / nsteps);
  if (ms_total) *ms_total = (float)(tot / nsteps);
  return ELMK_OK;
}
}  // namespace

extern "C" {

int elmk_frac_wet(elmk_ctx* ctx) { return launch_stage(ctx, TS7[ELMK_WRAPPER_FRAC_WET], 0.0); }
int elmk_albedo_snicar(elmk_ctx* ctx) { return launch_stage(ctx, TS7[ELMK_WRAPPER_ALBEDO_SNICAR], 0.0); }
int elmk_canopy_hydrology(elmk_ctx* ctx, double dt) { return launch_stage(ctx, TS7[ELMK_WRAPPER_CANOPY_HYDROLOGY], dt); }
int elmk_surface_radiation(elmk_ctx* ctx) { return launch_stage(ctx, TS7[ELMK_WRAPPER_SURFACE_RADIATION], 0.0); }
int elmk_canopy_temperature(elmk_ctx* ctx) { return launch_stage(ctx, TS7[ELMK_WRAPPER_CANOPY_TEMPERATURE], 0.0); }
int elmk_bareground_fluxes(elmk_ctx* ctx) { return launch_stage(ctx, TS7[ELMK_WRAPPER_BAREGROUND_FLUXES], 0.0); }
int elmk_canopy_fluxes(elmk_ctx* ctx, double dt) { return launch_stage(ctx, TS7[ELMK_WRAPPER_CANOPY_FLUXES], dt); }
int elmk_soil_temperature(elmk_ctx* ctx, double dt) { return launch_stage(ctx, SOIL_TEMPERATURE, dt); }
int elmk_snow_hydrology(elmk_ctx* ctx, double dt) { return launch_stage(ctx, SNOW_HYDROLOGY, dt); }
int elmk_surface_fluxes(elmk_ctx* ctx, double dt) { return launch_stage(ctx, SURFACE_FLUXES, dt); }

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// soil hydrology (k_soil_hydrology.hip; include/elmk.h "soil hydrology")
// ---------------------------------------------------------------------------------------------------
namespace {
bool hyd_land(const elmk_ctx* ctx) { return ctx->h.land.ltype == istsoil || ctx->h.land.ltype == istcrop; }
void hyd_launch(elmk_ctx* ctx, double dt)
{
  if (hyd_land(ctx)) launch_soil_hydrology(ctx->d, ctx->ncols, ctx->hyd_rows, dt, ctx->stream);
}
}  // namespace

extern "C" {

int elmk_soil_hydrology_enable(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (ctx->hyd_rows) return invalid(ctx, "elmk_soil_hydrology_enable: already enabled");
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_enable: the stream is being captured")) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its flags' moment)
  const size_t bytes = (size_t)ELMK_HYD_NROWS * (size_t)ctx->ld * sizeof(double);
  if (hip_fail(ctx, ctx->hyd_rows.alloc(bytes), "hipMalloc(soil hydrology rows)")) return ELMK_E_NOMEM;
  if (hip_fail(ctx, hipMemsetAsync(ctx->hyd_rows, 0, bytes, ctx->stream), "hipMemset(soil hydrology rows)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)ctx->hyd_rows.reset();
    return ELMK_E_HIP;
  }
  ctx->hyd_params = false;
  return ELMK_OK;
}

int elmk_soil_hydrology_set_params(elmk_ctx* ctx, const double* hksat, const double* wtfact, const double* h2osfc_thresh,
                                   const double* k_wet, const double* rsub_top_max)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_soil_hydrology_set_params: not enabled (elmk_soil_hydrology_enable)");
  if (!hksat || !wtfact || !h2osfc_thresh || !k_wet || !rsub_top_max) return invalid(ctx, "elmk_soil_hydrology_set_params: null argument");
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_set_params: the stream is being captured")) return rc;
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
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_soil_hydrology_init: not enabled (elmk_soil_hydrology_enable)");
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_init: the stream is being captured")) return rc;
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
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_soil_hydrology(elmk_ctx* ctx, double dt)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_soil_hydrology: not enabled (elmk_soil_hydrology_enable)");
  if (!ctx->hyd_params) return invalid(ctx, "elmk_soil_hydrology: the parameters are not set (elmk_soil_hydrology_set_params)");
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_soil_hydrology: dt must be finite and positive");
  if (int rc = enter_physics(ctx)) return rc;
  hyd_launch(ctx, dt);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_soil_hydrology_read(elmk_ctx* ctx, int which, double* host, int64_t col0, int64_t n)
{
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_soil_hydrology_read: not enabled (elmk_soil_hydrology_enable)");
  if (which < 0 || which >= ELMK_HYD_NROWS) return invalid(ctx, "elmk_soil_hydrology_read: unknown row");
  if ((!host && n > 0) || col0 < 0 || n < 0 || col0 + n > ctx->ncols) return invalid(ctx, "elmk_soil_hydrology_read: bad column range");
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_read: the stream is being captured")) return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->hyd_rows + (size_t)which * (size_t)ctx->ld + (size_t)col0, (size_t)n * 8, hipMemcpyDeviceToHost,
                          ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_soil_hydrology_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_soil_hydrology_clear: the stream is being captured")) return rc;
  if (!ctx->hyd_rows) return ELMK_OK;
  if (int rc = quiesce(ctx, false)) return rc;
  HIPCHK(ctx->hyd_rows.reset());
  ctx->hyd_params = false;
  return ELMK_OK;
}

}  // extern "C"

extern "C" {

// L2-level entries: the forcing-derived scalars handed in, as the reference's unit tests call the physics
// (test/test_CanFlux.cc:285-340, test/test_BGFlux.cc:200-260) instead of the wrapper's derive_forc_* (atm_physics_impl.hh:246-272)
namespace {
int stage_given(elmk_ctx* ctx, const double* rho, const double* po2, const double* pco2, int* mask)
{
  const double* src[3] = {rho, po2, pco2};
  *mask = 0;
  for (int k = 0; k < 3; k++) {
    if (!src[k] || ctx->ncols == 0) continue;
    HIPCHK(hipMemcpyAsync(ELMK_GENERIC(ctx->h.cf_given) + (size_t)k * ctx->ld, src[k], (size_t)ctx->ncols * 8, hipMemcpyHostToDevice,
                          ctx->stream));
    *mask |= 1 << k;
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));  // the sources are caller-owned pageable host arrays
  return ELMK_OK;
}
}  // namespace

int elmk_canopy_fluxes_given(elmk_ctx* ctx, double dt, const double* forc_rho, const double* forc_po2, const double* forc_pco2)
{
  if (int rc = enter_physics(ctx)) return rc;
  int mask = 0;
  if (int rc = stage_given(ctx, forc_rho, forc_po2, forc_pco2, &mask)) return rc;
  launch_canopy_fluxes(ctx->d, ctx->ncols, dt, ctx->stream, mask, &ctx->side);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_bareground_fluxes_given(elmk_ctx* ctx, const double* forc_rho)
{
  if (int rc = enter_physics(ctx)) return rc;
  int mask = 0;
  if (int rc = stage_given(ctx, forc_rho, nullptr, nullptr, &mask)) return rc;
  launch_bareground_fluxes(ctx->d, ctx->ncols, ctx->stream, mask);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_init_timestep(elmk_ctx* ctx)
{
  if (int rc = enter_physics(ctx)) return rc;
  launch_init_timestep(ctx->d, ctx->ncols, ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

}  // extern "C"

namespace {
// downscaling TOPO mode: the forcing kernels' parameters (ds_topo false: OFF, the kernels as they were)
bool ds_topo(const elmk_ctx* ctx) { return ctx->ds.mode == ELMK_DS_TOPO; }
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
}  // namespace

extern "C" {

int elmk_get_forcing(elmk_ctx* ctx, const double* wt1, const double* wt2, int qbot_is_rh)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (!wt1 || !wt2) return invalid(ctx, "elmk_get_forcing: null weights");
  const bool cz = ctx->sw.mode == ELMK_SW_COSZEN;
  if (cz && !ctx->sw.step_time)
    return invalid(ctx, "elmk_get_forcing: shortwave COSZEN mode needs the record's time (elmk_set_forcing_record_time)");
  const DsParams P = ds_params(ctx);
  launch_get_forcing(ctx->d, ctx->ncols, wt1, wt2, qbot_is_rh != 0, ctx->stream, cz ? (const double*)ctx->sw.czf : nullptr,
                     ds_topo(ctx) ? &P : nullptr);
  ds_lw_norm(ctx);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_phenology(elmk_ctx* ctx, double wt1, double wt2)
{
  if (int rc = enter_physics(ctx)) return rc;
  launch_phenology(ctx->d, ctx->ncols, wt1, wt2, ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_initialize_state(elmk_ctx* ctx)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (!ctx->have_init_params) return invalid(ctx, "elmk_initialize_state: elmk_set_init_params has not been called");
  launch_initialize_state(ctx->d, ctx->ncols, ctx->stream);
  HIPCHK(hipGetLastError());
  return ELMK_OK;
}

int elmk_evaluate_conservation(elmk_ctx* ctx, double dt, double* min_max_sum, double* per_column)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (!min_max_sum) return invalid(ctx, "elmk_evaluate_conservation: min_max_sum is NULL");
  const double* diag = ELMK_GENERIC(ctx->h.cons_diag);
  launch_conservation(ctx->d, ctx->ncols, ctx->ld, dt, diag, ctx->cons_part, ctx->cons_out, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(min_max_sum, ctx->cons_out, 8 * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (per_column) {  // [8][ncols], diagnostic-major
    for (int k = 0; k < 8; k++)
      HIPCHK(hipMemcpyAsync(per_column + (size_t)k * ctx->ncols, diag + (size_t)k * ctx->ld, (size_t)ctx->ncols * 8,
                            hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

int elmk_timestep7(elmk_ctx* ctx, double dt)
{
  if (int rc = enter_physics(ctx)) return rc;
  // ~22 dependent launches cost ~0.5 ms of launch latency however few columns there are; replaying them as one graph
  // removes the host side of that.  Kernel arguments are the device parameter block (fixed address) and dt.
  return launch_sequence(ctx, GRAPH_TS7, TS7, dt);
}

int elmk_timestep7_fused(elmk_ctx* ctx, double dt)
{
  if (int rc = enter_physics(ctx)) return rc;
  return launch_sequence(ctx, GRAPH_FUSED, FUSED, dt);
}

int elmk_advance_physics(elmk_ctx* ctx, double dt)
{
  if (int rc = enter_physics(ctx)) return rc;
  return launch_sequence(ctx, GRAPH_ADVANCE, ADVANCE, dt);
}

// ---------------------------------------------------------------------------------------------------
// multi-step runs: the driver's time loop (kokkos_driver.cc:54-85) on the device
// ---------------------------------------------------------------------------------------------------
namespace {
// quiesce and release the reservation: elmk_run_reserve, elmk_set_forcing_grid and elmk_clear_forcing_grid
int run_drop(elmk_ctx* ctx)
{
  if (int rc = quiesce(ctx, true)) return rc;
  ctx->run = elmk_ctx::Run{};
  return ELMK_OK;
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
void run_next(elmk_ctx* ctx, double) { launch_run_next(ctx->run.cursor, ctx->stream); }

// one model step of elmk_run, in the order of the stand-alone calls it replaces (include/elmk.h): solar geometry, phenology,
// forcing, aerosol deposition (ELMK_RUN_AEROSOL: where the reference's hook sits, init_timestep_kokkos.cc:48-49), init_timestep,
// advance_physics' stages, soil hydrology (ELMK_RUN_HYDROLOGY), conservation -> ring row, flag summary -> ring row, active layer thickness (ELMK_RUN_ALT), accumulated fields,
// history, next row
constexpr Stage RUN_STEP[] = {{run_solar_geometry, nullptr}, {run_phenology, nullptr},   {run_forcing, nullptr}, {run_aerosol, nullptr},
                              {run_init_timestep, nullptr},
                              ADVANCE[0], ADVANCE[1], ADVANCE[2], ADVANCE[3], ADVANCE[4], ADVANCE[5], ADVANCE[6], ADVANCE[7],
                              {run_soil_hydrology, nullptr},
                              {run_conservation, nullptr},   {run_flag_reduce, nullptr}, {run_active_layer, nullptr},
                              {run_accum, nullptr},          {run_history, nullptr},     {run_next, nullptr}};
static_assert(sizeof ADVANCE / sizeof ADVANCE[0] == 8, "RUN_STEP holds every stage of ADVANCE");
}  // namespace

int elmk_run_reserve(elmk_ctx* ctx, int forcing_slots, int max_steps)
{
  if (int rc = enter(ctx)) return rc;
  if (forcing_slots < 2 || forcing_slots > (1 << 20) || max_steps < 1 || max_steps > (1 << 24))
    return invalid(ctx, "elmk_run_reserve: need 2 <= forcing_slots <= 2^20 and 1 <= max_steps <= 2^24");
  if (int rc = refuse_capture(ctx, "elmk_run_reserve: the stream is being captured")) return rc;
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
  if (flags & ~(ELMK_RUN_QBOT_IS_RH | ELMK_RUN_HISTORY | ELMK_RUN_ACCUM | ELMK_RUN_AEROSOL | ELMK_RUN_ALT | ELMK_RUN_HYDROLOGY))
    return invalid(ctx, "elmk_run: unknown flags");
  if ((flags & ELMK_RUN_AEROSOL) && !ctx->aer.mem) return invalid(ctx, "elmk_run: ELMK_RUN_AEROSOL without an aerosol series (elmk_aerosol_reserve)");
  if ((flags & ELMK_RUN_ACCUM) && ctx->accum.empty()) return invalid(ctx, "elmk_run: ELMK_RUN_ACCUM without an accumulator entry (elmk_accum_add)");
  if ((flags & ELMK_RUN_ALT) && !ctx->alt_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_ALT without the active layer thickness enabled (elmk_active_layer_enable)");
  if ((flags & ELMK_RUN_HYDROLOGY) && !ctx->hyd_rows)
    return invalid(ctx, "elmk_run: ELMK_RUN_HYDROLOGY without the soil hydrology enabled (elmk_soil_hydrology_enable)");
  if ((flags & ELMK_RUN_HYDROLOGY) && !ctx->hyd_params)
    return invalid(ctx, "elmk_run: ELMK_RUN_HYDROLOGY without parameters (elmk_soil_hydrology_set_params)");
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
  if (int rc = refuse_capture(ctx, "elmk_run: the stream is being captured")) return rc;

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
  }
  const int row0 = buf * R.max_steps;
  HIPCHK(hipMemcpyAsync(R.table + row0, rows, (size_t)nsteps * sizeof(RunRow), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)R.cursor, row0, 1, ctx->stream));
  R.flags = flags;
  R.live[buf] = true;  // (from here on an upload of these records waits for the run's end event)
  R.slot_lo[buf] = lo;
  R.slot_hi[buf] = hi;
  R.months[buf] = months;
  R.aer_months[buf] = (flags & ELMK_RUN_AEROSOL) ? months : 0u;
  R.count++;
  R.last_buf = buf;
  R.last_nsteps = nsteps;
  // (the five flags below ELMK_RUN_HYDROLOGY: bits 5 .. 7 were taken before that flag existed)
  const uint64_t tag = (uint64_t)(flags & 31) | ((uint64_t)(ds_topo(ctx) && ctx->ds.gmem) << 5) | ((uint64_t)ds_topo(ctx) << 6) |
                       ((uint64_t)cz << 7) | ((ctx->hist_version & 0xFFFFFFFull) << 8) |  // bits 8..35 and 36..63: the tables'
                       ((ctx->accum_version & 0xFFFFFFFull) << 36);                       // versions, 28 bits each
  // the soil hydrology stage is in the captured step exactly when the run is flagged and the land unit is soil or crop
  const uint64_t tag2 = (flags & ELMK_RUN_HYDROLOGY) ? 1u + (uint64_t)hyd_land(ctx) : 0u;
  if (cz) {  // the run's czf replaces the stepwise record time's
    ctx->sw.step_time = false;
    ctx->sw.czf_ready = true;
  }
  int rc = ELMK_OK;
  for (int s = 0; s < nsteps && rc == ELMK_OK; s++) rc = launch_sequence(ctx, GRAPH_RUN_STEP, RUN_STEP, dt, tag, tag2);
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
  if (int rc = refuse_capture(ctx, "elmk_set_forcing_grid: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_clear_forcing_grid: the stream is being captured")) return rc;
  if (int rc = run_drop(ctx)) return rc;
  ctx->grid = elmk_ctx::Grid{};
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// aerosol deposition: a monthly climatology on a grid of its own, interpolated on the device (include/elmk.h "aerosol deposition")
// ---------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {
bool aerosol_field(int f) { return f >= ELMK_FIELD_aer_bcphi && f <= ELMK_FIELD_aer_dst4_2; }
}  // namespace

extern "C" {

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
  if (int rc = refuse_capture(ctx, "elmk_aerosol_reserve: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_aerosol_upload: the stream is being captured")) return rc;  // (it waits)
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
  if (int rc = refuse_capture(ctx, "elmk_aerosol_deposition: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_aerosol_clear: the stream is being captured")) return rc;
  if (int rc = quiesce(ctx, true)) return rc;
  ctx->aer = elmk_ctx::Aerosol{};
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// shortwave: interval-mean FSDS weighted by cos(zenith) (include/elmk.h "shortwave")
// ---------------------------------------------------------------------------------------------------
namespace {
// set the mode and forget every record time
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
bool rec_decday_ok(double d) { return d >= 0.0 && d < 1.0e9; }
}  // namespace

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
  if (int rc = refuse_capture(ctx, "elmk_set_shortwave_mode: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_series_record_times: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_download_forcing_cosz: the stream is being captured")) return rc;
  if (ctx->ncols > 0) HIPCHK(hipMemcpyAsync(czf, ctx->sw.czf, (size_t)ctx->ncols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// downscaling: forcing adjusted to each column's elevation (include/elmk.h "downscaling")
// ---------------------------------------------------------------------------------------------------
namespace {
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
}  // namespace

int elmk_set_column_elevation(elmk_ctx* ctx, const double* topo_col, const double* topo_forc)
{
  if (int rc = enter(ctx)) return rc;
  const int64_t n = ctx->ncols;
  if (!topo_col && n > 0) return invalid(ctx, "elmk_set_column_elevation: null topo_col");
  if (n > 0 && (!all_finite(topo_col, n) || (topo_forc && !all_finite(topo_forc, n))))
    return invalid(ctx, "elmk_set_column_elevation: non-finite elevation");
  if (int rc = refuse_capture(ctx, "elmk_set_column_elevation: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_set_forcing_elevation_gridded: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_set_downscaling: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_set_downscaling_groups: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_clear_downscaling_groups: the stream is being captured")) return rc;
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
  if (int rc = refuse_capture(ctx, "elmk_download_column_elevation: the stream is being captured")) return rc;
  const size_t bytes = (size_t)ctx->ncols * sizeof(double);
  if (topo_col && bytes) HIPCHK(hipMemcpyAsync(topo_col, D.topo, bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (topo_forc && bytes) HIPCHK(hipMemcpyAsync(topo_forc, D.topo + ctx->ld, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
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
  if (int rc = refuse_capture(ctx, "elmk_upload_gridded: the stream is being captured")) return rc;
  if (ctx->ncols == 0) return ELMK_OK;
  char* dst = (char*)ctx->fptr[field] + (size_t)level * (size_t)ctx->ld * (size_t)store_size(ELMK_F64);
  // staging is reused by the next call: the copy and the remap are done when this returns, as elmk_upload's copy is
  HIPCHK(hipMemcpyAsync(G.cells, cells, (size_t)G.map.ncells * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  launch_remap_field(dst, G.cells, ctx->ncols, ctx->ld, G.map.npad, G.map.idx, G.map.w, ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

// ---------------------------------------------------------------------------------------------------
// output grid: columns aggregated onto cells on the device through a CSR map (include/elmk.h "output grid")
// ---------------------------------------------------------------------------------------------------
int elmk_set_output_grid(elmk_ctx* ctx, int64_t ncells, const int64_t* ptr, const int32_t* col, const double* w, double fill)
{
  if (int rc = enter(ctx)) return rc;
  // (every gather of the aggregate kernels stays inside a source row because of this check)
  if (int rc = invalid_map(ctx, "elmk_set_output_grid", csr_check(ncells, ctx->ncols, ptr, col, w, "ncells outside 1 .. 2^31-1", false, false))) return rc;
  if (int rc = refuse_capture(ctx, "elmk_set_output_grid: the stream is being captured")) return rc;
  if (has_gridded_entries(ctx)) return invalid(ctx, "elmk_set_output_grid: gridded history entries exist (elmk_history_clear first)");
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
  if (int rc = refuse_capture(ctx, "elmk_clear_output_grid: the stream is being captured")) return rc;
  if (has_gridded_entries(ctx)) return invalid(ctx, "elmk_clear_output_grid: gridded history entries exist (elmk_history_clear first)");
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
  if (int rc = refuse_capture(ctx, "elmk_download_gridded: the stream is being captured")) return rc;
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

// ---------------------------------------------------------------------------------------------------
// diagnostics
// ---------------------------------------------------------------------------------------------------
int elmk_error_summary(elmk_ctx* ctx, uint32_t* or_of_flags, int64_t* first_bad_col)
{
  if (int rc = enter(ctx)) return rc;
  const long long none = 0x7fffffffffffffffll;
  HIPCHK(hipMemsetAsync(ctx->red_or, 0, 8, ctx->stream));
  HIPCHK(hipMemcpyAsync(ctx->red_first, &none, 8, hipMemcpyHostToDevice, ctx->stream));
  launch_flag_reduce((const uint32_t*)ctx->fptr[ELMK_FIELD_err_flags], ctx->ncols, ctx->red_or, ctx->red_first,
                     ctx->stream);
  HIPCHK(hipGetLastError());
  uint32_t o = 0;
  long long first = none;
  HIPCHK(hipMemcpyAsync(&o, ctx->red_or, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipMemcpyAsync(&first, ctx->red_first, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (or_of_flags) *or_of_flags = o;
  if (first_bad_col) *first_bad_col = (first == none) ? -1 : (int64_t)first;
  return ELMK_OK;
}

int elmk_clear_errors(elmk_ctx* ctx) { return elmk_fill(ctx, ELMK_FIELD_err_flags, 0.0); }

int elmk_profile_timestep7(elmk_ctx* ctx, double dt, int nsteps, float* ms_per_kernel, float* ms_total)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (nsteps <= 0) return invalid(ctx, "elmk_profile_timestep7: nsteps <= 0");
  return profile_stages(ctx, TS7, dt, nsteps, true, nullptr, ms_per_kernel, ms_total, nullptr);
}

int elmk_profile_timestep7_fused(elmk_ctx* ctx, double dt, int nsteps, float* ms_per_stage, float* ms_total)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (nsteps <= 0) return invalid(ctx, "elmk_profile_timestep7_fused: nsteps <= 0");
  return profile_stages(ctx, FUSED, dt, nsteps, true, nullptr, ms_per_stage, ms_total, nullptr);
}

int elmk_profile_steps(elmk_ctx* ctx, int fused, double dt, int nsteps, float* ms_each_step)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (nsteps <= 0 || !ms_each_step) return invalid(ctx, "elmk_profile_steps: bad arguments");
  return profile_stages(ctx, fused ? Stages(FUSED) : Stages(TS7), dt, nsteps, true, nullptr, nullptr, nullptr, ms_each_step);
}

int elmk_profile_wrapper(elmk_ctx* ctx, int wrapper, double dt, int nsteps, float* ms_mean)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (nsteps <= 0 || !ms_mean) return invalid(ctx, "elmk_profile_wrapper: bad arguments");
  if (wrapper < 0 || wrapper > ELMK_WRAPPER_ADVANCE_PHYSICS) return invalid(ctx, "elmk_profile_wrapper: unknown wrapper");
  const Stages L = wrapper <= ELMK_WRAPPER_CANOPY_FLUXES       ? Stages(TS7[wrapper])
                   : wrapper == ELMK_WRAPPER_SOIL_TEMPERATURE ? Stages(SOIL_TEMPERATURE)
                   : wrapper == ELMK_WRAPPER_SNOW_HYDROLOGY   ? Stages(SNOW_HYDROLOGY)
                   : wrapper == ELMK_WRAPPER_SURFACE_FLUXES   ? Stages(SURFACE_FLUXES)
                                                              : Stages(ADVANCE);
  const char* label = wrapper == ELMK_WRAPPER_SOIL_TEMPERATURE ? "kokkos_soil_temperature"
                      : wrapper == ELMK_WRAPPER_SNOW_HYDROLOGY ? "kokkos_snow_hydrology"
                      : wrapper == ELMK_WRAPPER_SURFACE_FLUXES ? "kokkos_surface_fluxes"
                                                               : "elmk_wrapper";
  // one event pair per step around the whole wrapper: bench.py times advance_physics with it, and events between its stages
  // would change what it measures
  return profile_stages(ctx, L, dt, nsteps, false, label, nullptr, ms_mean, nullptr);
}

int elmk_read_scratch(elmk_ctx* ctx, int kind, void* host, int64_t offset, int64_t count)
{
  if (int rc = enter(ctx)) return rc;
  if (!host || offset < 0 || count < 0) return invalid(ctx, "elmk_read_scratch: bad arguments");
  const void* src = nullptr;
  size_t esz = 0;
  int64_t limit = 0;
  if (kind == ELMK_SCRATCH_LIST_COUNTS) {  // (count, head) of every work list: the counters sit one per 128-byte line
    if (offset != 0 || count != 2 * NLISTS) return invalid(ctx, "elmk_read_scratch: the list counters are read whole (2 x the number of lists)");
    std::vector<uint32_t> raw((size_t)2 * NLISTS * CPAD);
    HIPCHK(hipMemcpyAsync(raw.data(), ELMK_GENERIC(ctx->h.counters), raw.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < NLISTS; k++) {
      ((uint32_t*)host)[2 * k] = raw[(size_t)k * CPAD];
      ((uint32_t*)host)[2 * k + 1] = raw[(size_t)(NLISTS + k) * CPAD];
    }
    return ELMK_OK;
  }
  if (kind == ELMK_SCRATCH_CF_TRIPS || kind == ELMK_SCRATCH_CF_HINTS) {
    src = ELMK_GENERIC(ctx->h.cf_niter);
    esz = 4;
    limit = ctx->ncols;
  } else if (kind == ELMK_SCRATCH_WORK) {
    src = ELMK_GENERIC(ctx->h.wk);
    esz = 8;
    limit = (int64_t)WK_N * ctx->ld;
  } else {
    return invalid(ctx, "elmk_read_scratch: unknown kind");
  }
  if (offset + count > limit) return invalid(ctx, "elmk_read_scratch: range exceeds the scratch array");
  HIPCHK(hipMemcpyAsync(host, (const char*)src + (size_t)offset * esz, (size_t)count * esz, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (kind == ELMK_SCRATCH_CF_TRIPS)  // the high half of each word is the scheduler's hint
    for (int64_t i = 0; i < count; i++) ((int32_t*)host)[i] &= 0xFFFF;
  if (kind == ELMK_SCRATCH_CF_HINTS)
    for (int64_t i = 0; i < count; i++) ((int32_t*)host)[i] >>= 16;
  return ELMK_OK;
}

int elmk_state_real_bytes(void) { return kStateF32 ? 4 : 8; }

int elmk_copy_bandwidth(elmk_ctx* ctx, int64_t bytes, int iters, double* gbytes_per_s)
{
  return elmk_copy_bandwidth_shape(ctx, bytes, iters, 0, gbytes_per_s);
}

int elmk_copy_bandwidth_shape(elmk_ctx* ctx, int64_t bytes, int iters, int shape, double* gbytes_per_s)
{
  if (int rc = enter(ctx)) return rc;
  if (bytes < 512 || iters <= 0 || shape < 0 || shape > 4 || !gbytes_per_s) return invalid(ctx, "elmk_copy_bandwidth: bad arguments");
  const int64_t n = (bytes / 512) * 64;  // whole 512-byte runs: every shape copies the same bytes
  DevBuf<double> a, b;
  if (hip_fail(ctx, a.alloc((size_t)n * 8), "hipMalloc") || hip_fail(ctx, b.alloc((size_t)n * 8), "hipMalloc")) return ELMK_E_NOMEM;
  EventList ev;
  HIPCHK(ev.create(2));
  HIPCHK(hipMemsetAsync(a, 0, (size_t)n * 8, ctx->stream));
  launch_copy(a, b, n, ctx->stream, shape);  // warm-up
  HIPCHK(hipEventRecord(ev[0], ctx->stream));
  for (int i = 0; i < iters; i++) launch_copy(a, b, n, ctx->stream, shape);
  HIPCHK(hipEventRecord(ev[1], ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  *gbytes_per_s = 2.0 * (double)n * 8.0 * iters / ((double)ms * 1e-3) / 1e9;
  return ELMK_OK;
}

int elmk_math_eval(elmk_ctx* ctx, int fn, const double* x, const double* y, double* out, int64_t n)
{
  if (int rc = enter(ctx)) return rc;
  const bool binary = fn == ELMK_MATH_DIV || fn == ELMK_MATH_POW;
  if (fn < ELMK_MATH_EXP || fn > ELMK_MATH_SIN || !x || !out || n < 0 || (binary && !y))
    return invalid(ctx, "elmk_math_eval: bad arguments");
  if (n == 0) return ELMK_OK;
  DevBuf<double> d;
  if (hip_fail(ctx, d.alloc((size_t)n * 8 * 3), "hipMalloc")) return ELMK_E_HIP;
  if (hip_fail(ctx, hipMemcpyAsync(d, x, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync")) return ELMK_E_HIP;
  if (binary && hip_fail(ctx, hipMemcpyAsync(d + n, y, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream), "hipMemcpyAsync"))
    return ELMK_E_HIP;
  launch_math_eval(fn, d, d + n, d + 2 * n, n, ctx->stream);
  if (hip_fail(ctx, hipMemcpyAsync(out, d + 2 * n, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"))
    return ELMK_E_HIP;
  return ELMK_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------
// restart images (k_restart.hip; include/elmk.h "restart")
// ---------------------------------------------------------------------------------------------------
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
int field_class(int f) { return g_class.c[f]; }

constexpr size_t RST_ALIGN = 256;
constexpr size_t RST_CHUNK = (size_t)64 << 20;  // bytes of image per staging chunk
constexpr int RST_MAX_PIECES = 8192;            // per chunk (grid.y)

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
  std::vector<elmk_restart_accum> acc;  // version 2: one per accumulator entry (nsteps filled in by the save)
  std::vector<elmk_restart_section> sec;
  std::vector<RstSrc> src;
  bool hyd = false;  // version 4: the soil hydrology is enabled (the count word is present, the ZWT and WA sections last)
  bool alt = false;  // version 3: the active layer thickness is enabled (the accumulator-count word is present, three ALT sections last)
  size_t header_bytes = 0, total = 0;
};

int image_esize(int dtype) { return dtype == ELMK_F64 ? 8 : (dtype == ELMK_U8 ? 1 : 4); }

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
    const int64_t ext = e.cells ? ctx->ogrid.map.nrows : ctx->ncols;
    L.ent.push_back(elmk_restart_entry{e.tape, e.field, e.op, e.cells ? 1 : 0, e.cells ? ctx->ogrid.map.nrows : 0});
    L.sec.push_back(elmk_restart_section{e.cells ? ELMK_RESTART_GRIDDED : ELMK_RESTART_HISTORY, (int32_t)i, e.nlev, ELMK_F64, ext, 0, 0});
    L.src.push_back(RstSrc{(char*)(double*)e.acc, e.cld, ELMK_F64, e.cells ? 0 : gcol0, false});
  }
  for (size_t i = 0; i < ctx->accum.size(); i++) {
    const elmk_ctx::AccumEntry& e = ctx->accum[i];
    L.acc.push_back(elmk_restart_accum{e.src, e.kind, e.dst, 0, e.period, 0});
    L.sec.push_back(elmk_restart_section{ELMK_RESTART_ACCUM, (int32_t)i, e.nlev, ELMK_F64, ctx->ncols, 0, 0});
    L.src.push_back(RstSrc{(char*)(double*)e.val, ctx->ld, ELMK_F64, gcol0, false});
  }
  L.alt = (bool)ctx->alt_rows;
  for (int which = 0; L.alt && which < ALT_NROWS; which++) {
    L.sec.push_back(elmk_restart_section{ELMK_RESTART_ALT, which, 1, ELMK_F64, ctx->ncols, 0, 0});
    L.src.push_back(RstSrc{(char*)(ctx->alt_rows + (size_t)which * (size_t)ctx->ld), ctx->ld, ELMK_F64, gcol0, false});
  }
  L.hyd = (bool)ctx->hyd_rows;
  for (int which = ELMK_HYD_ZWT; L.hyd && which <= ELMK_HYD_WA; which++) {
    L.sec.push_back(elmk_restart_section{ELMK_RESTART_HYDROLOGY, which, 1, ELMK_F64, ctx->ncols, 0, 0});
    L.src.push_back(RstSrc{(char*)(ctx->hyd_rows + (size_t)which * (size_t)ctx->ld), ctx->ld, ELMK_F64, gcol0, false});
  }
  // version 2 (with accumulator entries), 3 and 4: their number in the word after the header, their table after the history entries
  L.header_bytes = align_up(sizeof(elmk_restart_header) + (L.acc.empty() && !L.alt && !L.hyd ? 0 : 8 + L.acc.size() * sizeof(elmk_restart_accum)) +
                                L.ent.size() * sizeof(elmk_restart_entry) + L.sec.size() * sizeof(elmk_restart_section),
                            RST_ALIGN);
  size_t off = L.header_bytes;
  for (elmk_restart_section& s : L.sec) {
    s.offset = off;
    off = align_up(off + (size_t)s.nlev * (size_t)s.extent * image_esize(s.dtype), RST_ALIGN);
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
    const int es = image_esize(S.dtype);
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
  if (int rc = refuse_capture(ctx, (std::string(who) + ": the stream is being captured").c_str())) return rc;
  HIPCHK(hipStreamSynchronize(ctx->stream));  // every elmk_run and accumulate in flight
  return ELMK_OK;
}
}  // namespace

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
    const size_t end = s.offset + (size_t)s.nlev * (size_t)s.extent * image_esize(s.dtype);
    memset(out + end, 0, align_up(end, RST_ALIGN) - end);
  }
  elmk_restart_header H{};
  memcpy(H.magic, ELMK_RESTART_MAGIC, 8);
  H.version = L.hyd ? ELMK_RESTART_VERSION_HYDROLOGY : L.alt ? ELMK_RESTART_VERSION_ALT : L.acc.empty() ? ELMK_RESTART_VERSION : ELMK_RESTART_VERSION_ACCUM;
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
  if (!L.acc.empty() || L.alt || L.hyd) {
    const uint32_t word[2] = {(uint32_t)L.acc.size(), 0u};
    memcpy(p, word, 8);
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
  if (memcmp(H.magic, ELMK_RESTART_MAGIC, 8) != 0 || (H.version != ELMK_RESTART_VERSION && H.version != ELMK_RESTART_VERSION_ACCUM && H.version != ELMK_RESTART_VERSION_ALT &&
                                                 H.version != ELMK_RESTART_VERSION_HYDROLOGY))
    return invalid(ctx, "elmk_restart_load: not a restart image of this format version");
  if (H.header_bytes > (uint64_t)bytes || H.total_bytes > (uint64_t)bytes || H.header_bytes % 8 != 0)
    return invalid(ctx, "elmk_restart_load: truncated image");
  if (header_checksum(in, H.header_bytes) != H.header_checksum) return invalid(ctx, "elmk_restart_load: header checksum mismatch");
  if (H.schema_hash != schema_hash()) return invalid(ctx, "elmk_restart_load: the image was saved with another field schema");
  if (H.ncols != ctx->ncols) return invalid(ctx, "elmk_restart_load: the image holds another number of columns");
  if (H.gcol0 != gcol0) return invalid(ctx, "elmk_restart_load: the image starts at another global column");
  const RstLayout L = rst_layout(ctx, gcol0);
  // the accumulator table first (version 2 holds one, and only a context with entries saves or loads version 2)
  const unsigned char* p = in + sizeof H;
  unsigned long long nacc[ELMK_ACCUM_MAX_ENTRIES] = {};
  const char* const acc_differs = "elmk_restart_load: the image's accumulator entries differ from the context's";
  // (version 3 is what a context with the active layer thickness saves and loads, with or without accumulator entries)
  // (version 4 is what a context with the soil hydrology saves and loads; whether it holds the ALT sections too is the section table's to say)
  if ((H.version == ELMK_RESTART_VERSION_HYDROLOGY) != L.hyd)
    return invalid(ctx, L.hyd ? "elmk_restart_load: the soil hydrology is enabled and the image holds none (version 1 to 3)"
                              : "elmk_restart_load: a version-4 image needs the soil hydrology enabled (elmk_soil_hydrology_enable)");
  if (!L.hyd && (H.version == ELMK_RESTART_VERSION_ALT) != L.alt)
    return invalid(ctx, L.alt ? "elmk_restart_load: the active layer thickness is enabled and the image holds none (version 1 or 2)"
                              : "elmk_restart_load: a version-3 image needs the active layer thickness enabled (elmk_active_layer_enable)");
  if (!L.alt && !L.hyd && (H.version == ELMK_RESTART_VERSION_ACCUM) != !L.acc.empty()) return invalid(ctx, acc_differs);
  if (!L.acc.empty() || L.alt || L.hyd) {
    uint32_t word[2];
    if (H.header_bytes < sizeof H + 8) return invalid(ctx, "elmk_restart_load: truncated image");
    memcpy(word, p, 8);
    if (word[0] != L.acc.size() || word[1] != 0u) return invalid(ctx, acc_differs);
    p += 8;
  }
  if (L.hyd) {
    // a version-4 image says in its section table whether it holds the active layer rows too: the enabled features must match
    const size_t at = (size_t)(p - in) + (size_t)H.nentries * sizeof(elmk_restart_entry) + L.acc.size() * sizeof(elmk_restart_accum);
    if (at > H.header_bytes || (H.header_bytes - at) / sizeof(elmk_restart_section) < H.nsections)
      return invalid(ctx, "elmk_restart_load: truncated image");
    bool alt = false;
    for (uint32_t k = 0; k < H.nsections; k++) {
      elmk_restart_section S;
      memcpy(&S, in + at + (size_t)k * sizeof S, sizeof S);
      alt = alt || S.kind == ELMK_RESTART_ALT;
    }
    if (alt != L.alt)
      return invalid(ctx, L.alt ? "elmk_restart_load: the active layer thickness is enabled and the version-4 image holds no such rows"
                                : "elmk_restart_load: the version-4 image holds active layer rows and the feature is not enabled (elmk_active_layer_enable)");
  }
  if (H.nentries != L.ent.size() || H.nsections != L.sec.size() || H.header_bytes != L.header_bytes || H.total_bytes != L.total)
    return invalid(ctx, "elmk_restart_load: the image's history entries differ from the context's");
  for (size_t i = 0; i < L.ent.size(); i++) {
    elmk_restart_entry E;
    memcpy(&E, p + i * sizeof E, sizeof E);
    if (memcmp(&E, &L.ent[i], sizeof E) != 0) return invalid(ctx, "elmk_restart_load: the image's history entries differ from the context's");
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
  // pass 1: every checksum and the snl range, state untouched
  const int nch = (int)P.lo.size();
  for (int k = 0; k < nch; k++) {
    HIPCHK(hipMemcpyAsync(R.stage, in + P.lo[k], P.hi[k] - P.lo[k], hipMemcpyHostToDevice, ctx->stream));
    launch_restart_pieces(1, (RstPiece*)R.table + P.first[k], P.first[k + 1] - P.first[k], P.nbx[k], R.stage, R.part,
                          (uint64_t*)R.sums + 2 * (size_t)P.first[k], ctx->stream);
    HIPCHK(hipGetLastError());
  }
  std::vector<uint64_t> sums(2 * P.pieces.size());
  if (!sums.empty()) HIPCHK(hipMemcpyAsync(sums.data(), R.sums, sums.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  std::vector<uint64_t> ck;
  uint64_t bad = 0;
  section_sums(P, sums, L.sec.size(), ck, &bad);
  for (size_t s = 0; s < L.sec.size(); s++)
    if (ck[s] != want[s]) return invalid(ctx, "elmk_restart_load: section checksum mismatch");
  if (bad) return invalid(ctx, "elmk_restart_load: snl outside 0..nlevsno");
  // pass 2: scatter into the state and the accumulators, then the tape counts
  for (int k = 0; k < nch; k++) {
    HIPCHK(hipMemcpyAsync(R.stage, in + P.lo[k], P.hi[k] - P.lo[k], hipMemcpyHostToDevice, ctx->stream));
    launch_restart_pieces(2, (RstPiece*)R.table + P.first[k], P.first[k + 1] - P.first[k], P.nbx[k], R.stage, R.part, nullptr,
                          ctx->stream);
    HIPCHK(hipGetLastError());
  }
  if (ctx->hist_table) {
    unsigned long long counts[ELMK_HIST_MAX_TAPES];
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++) counts[t] = H.tape_count[t];
    HIPCHK(hipMemcpyAsync(hist_counts(ctx), counts, sizeof counts, hipMemcpyHostToDevice, ctx->stream));
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++) ctx->hist_dirty[t] = counts[t] > 0;
  }
  if (!L.acc.empty())
    HIPCHK(hipMemcpyAsync(accum_counts(ctx), nacc, L.acc.size() * sizeof nacc[0], hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return ELMK_OK;
}

}  // extern "C"
