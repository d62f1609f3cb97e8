// elmk_api.cpp - host side of the C ABI declared in include/elmk.h.
//
// Owns the device arena (every field of elmk_fields.def as SoA [lev][column], level stride padded to 64
// columns, each field 256-byte aligned), the parameter block (DevState) mirrored into device memory, one
// HIP stream, and a staging buffer for layout conversion.  No physics lives here and there is no CPU path:
// every elmk_<physics>() is a single kernel launch on the context's stream.
// The optional run features live in api_history.cpp, api_accum.cpp, api_rows.cpp, api_irrigation.cpp, api_routing.cpp, api_run.cpp and api_restart.cpp; elmk_ctx.h is what
// they share.
#include "elmk_ctx.h"

#include <dlfcn.h>

namespace {

thread_local std::string g_create_error;

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

}  // namespace

namespace elmk {

const FieldDesc g_fields[ELMK_NUM_FIELDS] = {
#define ELMK_FIELD(name, T, nlev) {#name, ELMK_##T, nlev},
#include "elmk_fields.def"
#undef ELMK_FIELD
    {"err_flags", ELMK_U32, 1},
};

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

int launched(elmk_ctx* ctx) { return hip_fail(ctx, hipGetLastError(), "hipGetLastError()") ? ELMK_E_HIP : ELMK_OK; }
int synced(elmk_ctx* ctx) { return hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize(ctx->stream)") ? ELMK_E_HIP : ELMK_OK; }

int invalid_map(elmk_ctx* ctx, const char* who, const char* text)
{
  return text ? invalid(ctx, (std::string(who) + ": " + text).c_str()) : ELMK_OK;
}

int check_range(elmk_ctx* ctx, const char* who, const void* host, int64_t col0, int64_t n, int64_t lim, const char* what)
{
  if ((host || n <= 0) && col0 >= 0 && n >= 0 && col0 + n <= lim) return ELMK_OK;
  return invalid(ctx, (std::string(who) + ": bad " + what + " range").c_str());
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

int refuse_capture(elmk_ctx* ctx, const char* who)
{
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hip_fail(ctx, hipStreamIsCapturing(ctx->stream, &cap), "hipStreamIsCapturing")) return ELMK_E_HIP;
  return cap != hipStreamCaptureStatusNone ? invalid(ctx, (std::string(who) + ": the stream is being captured").c_str()) : ELMK_OK;
}

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

// Columns [col0, col0 + n) of nlev device rows, ld elements of es bytes apart, from (up) or to the host's n > 0 columns: as rows of n
// elements (ELMK_LAYOUT_SOA, or one level), else in the reference layout [col][lev] through the device staging buffer in chunks of
// whole 64-column tiles.  Enqueued on the context's stream, which is waited for only where a chunk reuses the staging buffer: the
// caller waits for the end (the host side is pageable memory).
int xfer_rows(elmk_ctx* ctx, char* dev, int64_t ld, int es, int nlev, void* host, int64_t col0, int64_t n, int layout, bool up)
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

// the run step's form of the sequence: with ELMK_RUN_IRRIGATION the irrigation stage goes between the last fused group and
// soil_temperature ("irrigation": the stepwise placement); elmk_advance_physics itself never irrigates
void launch_advance(elmk_ctx* ctx, double dt)
{
  for (int k = 0; k < ELMK_FUSED_NSTAGE; k++) launch(ctx, ADVANCE[k], dt);
  if (ctx->run.flags & ELMK_RUN_IRRIGATION) irr_run_launch(ctx, dt);
  for (size_t k = ELMK_FUSED_NSTAGE; k < sizeof ADVANCE / sizeof ADVANCE[0]; k++) launch(ctx, ADVANCE[k], dt);
}

// the stages in order; marks (may be null): events recorded on the context's stream before the first stage and after the last,
// and with per_stage before every stage (marks[k] before stage k)
int enqueue_stages(elmk_ctx* ctx, Stages L, double dt, hipEvent_t* marks, bool per_stage)
{
  for (int k = 0; k < L.n; k++) {
    if (marks && (per_stage || k == 0)) HIPCHK(hipEventRecord(marks[k], ctx->stream));
    launch(ctx, L.s[k], dt);
  }
  if (marks) HIPCHK(hipEventRecord(marks[per_stage ? L.n : 1], ctx->stream));
  return launched(ctx);
}

// the stages captured once as a HIP graph (kernel nodes in one chain: the side-stream forks are issued in order on the
// capturing stream) and replayed
int run_graph(elmk_ctx* ctx, GraphSlot& g, Stages L, double dt, const StepKey& key)
{
  if (!g.exec || g.dt != dt || g.stream != ctx->stream || !(g.key == key)) {
    if (g.exec) {
      // dt, the stream or the key changed: the old executable may still be running its last launch.  (Best effort: a caller that
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
    g.key = key;
  }
  HIPCHK(hipGraphLaunch(g.exec, ctx->stream));
  return ELMK_OK;
}

int launch_sequence(elmk_ctx* ctx, GraphId id, Stages L, double dt, const StepKey& key)
{
  if (ctx->use_graph) return run_graph(ctx, ctx->graph[id], L, dt, key);
  return enqueue_stages(ctx, L, dt);
}

}  // namespace elmk

namespace {

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

// host elements already in the stored element type
int xfer_stored(elmk_ctx* ctx, int field, void* host, int64_t col0, int64_t n, int layout, bool up)
{
  const int nlev = g_fields[field].nlev;
  if (layout != ELMK_LAYOUT_SOA && layout != ELMK_LAYOUT_COL_MAJOR && nlev != 1) return invalid(ctx, "elmk_upload/download: unknown layout");
  if (int rc = xfer_rows(ctx, (char*)ctx->fptr[field], ctx->ld, store_size(g_fields[field].dtype), nlev, host, col0, n, layout, up)) return rc;
  return synced(ctx);
}

int xfer(elmk_ctx* ctx, int field, void* host, int64_t col0, int64_t n, int layout, bool up)
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

// L2-level entries: the forcing-derived scalars handed in, as the reference's unit tests call the physics
// (test/test_CanFlux.cc:285-340, test/test_BGFlux.cc:200-260) instead of the wrapper's derive_forc_* (atm_physics_impl.hh:246-272)
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
  return synced(ctx);  // the sources are caller-owned pageable host arrays
}
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
  if (option == ELMK_OPT_RESTART_CELLS) {  // (no launch depends on it: the captured graphs stay)
    if (int rc = refuse_capture(ctx, "elmk_set_option")) return rc;
    ctx->restart_cells = value != 0;
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
  return synced(ctx);
}

int64_t elmk_ncols(const elmk_ctx* ctx) { return ctx ? ctx->ncols : -1; }
int64_t elmk_level_stride(const elmk_ctx* ctx) { return ctx ? ctx->ld : -1; }
int64_t elmk_device_bytes(const elmk_ctx* ctx)
{
  if (!ctx) return -1;
  size_t n = ctx->arena.bytes() + ctx->staging.bytes() + ctx->scratch.bytes() + ctx->snicar.bytes() + ctx->snowage.bytes() + ctx->d.bytes() +
             ctx->run.mem.bytes() + ctx->grid.mem.bytes() + ctx->ogrid.mem.bytes() + ctx->sw.czf.bytes() + ctx->run.rec.bytes() +
             ctx->ds.topo.bytes() + ctx->ds.gmem.bytes() + ctx->accum_table.bytes() + ctx->aer.mem.bytes() + ctx->alt_rows.bytes() +
             ctx->hyd_rows.bytes() + ctx->hydf_rows.bytes() + ctx->hs.mem.bytes() + ctx->wb_rows.bytes() + ctx->wb_red.bytes() + ctx->wb_ring.bytes() +
             ctx->irr_rows.bytes() + route_bytes(ctx) + ctx->irrsup_rows.bytes() + ctx->pts.mem.bytes() + ctx->pts.ring.bytes() +
             ctx->pts.stamps.bytes();
  // the cell rows of gridded history entries (not the column rows) and the accumulators' values: whole rows of ld or cld doubles,
  // both multiples of 64, so every size is a multiple of 256 already
  for (const elmk_ctx::HistEntry& e : ctx->hist) n += e.cells || e.cellrow ? e.acc.bytes() : 0;  // (a cell-row entry's are cell rows too)
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
  return launched(ctx);
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
  return launched(ctx);
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
  return launched(ctx);
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
  return launched(ctx);
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
  return synced(ctx);
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
  return synced(ctx);
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
// physics wrappers: one launch each, same order/arguments as driver/kokkos
// ---------------------------------------------------------------------------------------------------
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

int elmk_canopy_fluxes_given(elmk_ctx* ctx, double dt, const double* forc_rho, const double* forc_po2, const double* forc_pco2)
{
  if (int rc = enter_physics(ctx)) return rc;
  int mask = 0;
  if (int rc = stage_given(ctx, forc_rho, forc_po2, forc_pco2, &mask)) return rc;
  launch_canopy_fluxes(ctx->d, ctx->ncols, dt, ctx->stream, mask, &ctx->side);
  return launched(ctx);
}

int elmk_bareground_fluxes_given(elmk_ctx* ctx, const double* forc_rho)
{
  if (int rc = enter_physics(ctx)) return rc;
  int mask = 0;
  if (int rc = stage_given(ctx, forc_rho, nullptr, nullptr, &mask)) return rc;
  launch_bareground_fluxes(ctx->d, ctx->ncols, ctx->stream, mask);
  return launched(ctx);
}

int elmk_init_timestep(elmk_ctx* ctx)
{
  if (int rc = enter_physics(ctx)) return rc;
  launch_init_timestep(ctx->d, ctx->ncols, ctx->stream);
  return launched(ctx);
}

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
  return launched(ctx);
}

int elmk_phenology(elmk_ctx* ctx, double wt1, double wt2)
{
  if (int rc = enter_physics(ctx)) return rc;
  launch_phenology(ctx->d, ctx->ncols, wt1, wt2, ctx->stream);
  return launched(ctx);
}

int elmk_initialize_state(elmk_ctx* ctx)
{
  if (int rc = enter_physics(ctx)) return rc;
  if (!ctx->have_init_params) return invalid(ctx, "elmk_initialize_state: elmk_set_init_params has not been called");
  launch_initialize_state(ctx->d, ctx->ncols, ctx->stream);
  return launched(ctx);
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
  return synced(ctx);
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
