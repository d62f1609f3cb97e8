// elmk_ctx.h - the context behind the C ABI and what the host units of the library share (elmk_api.cpp, api_*.cpp).  Host only: no
// kernel unit includes it.
#pragma once
#include "elmk.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_maps.h"

struct elmk_ctx;

namespace elmk {

struct FieldDesc {
  const char* name;
  int dtype;
  int nlev;
};
extern const FieldDesc g_fields[ELMK_NUM_FIELDS];
inline bool field_ok(int f) { return f >= 0 && f < ELMK_NUM_FIELDS; }
int field_class(int f);  // include/elmk_restart.def (api_restart.cpp)

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

// What the captured launches of a sequence depend on besides (dt, stream).  elmk_run's step: the run's flags, the downscaling and
// shortwave modes, whether the soil hydrology stage is in the step (its flag is set and the land unit is soil or crop), whether that
// stage takes the frost-table form, the history and accumulator tables' versions, whether the irrigation stage is in the step (its flag
// is set and the land unit is soil or crop), whether the water balance takes its term, whether the routing stage takes the withdrawal and
// whether the irrigation stage has the river supply limit's launch behind it, and whether the point series' record follows the history;
// the other sequences have none (StepKey{}).
struct StepKey {
  int flags = 0;
  bool ds_topo = false, ds_groups = false, coszen = false, hyd_stage = false, hyd_frost = false;
  uint64_t hist_version = 0, accum_version = 0;
  bool irr_stage = false, wb_irrig = false;  // the irrigation stage is in the step; the water balance takes the irrigation's term
  bool route_withdraw = false;               // the routing stage is in the step (its flag) and subtracts the irrigation's withdrawal
  bool irr_supply = false;                   // the irrigation stage is in the step and the river supply limit's launch follows it
  bool route_dam = false;                    // the routing stage is in the step and takes the reservoirs' form (its time from the pad word)
  bool route_heat = false;                   // the routing stage is in the step and takes the stream temperature's form
  bool land = false;                         // the floodplain infiltration is on: the hydrology, water balance and routing stages take its forms
  bool route_cmd = false;                    // the command areas are on: the routing stage has their two launches, the supply limit their form
  uint64_t points_version = 0;               // the point series is armed: its launch follows the history's (its version; 0: not armed)
  bool hyd_lat = false;                      // the hydrology stage is in the step and takes the hillslope lateral flow's form and launches
  auto tie() const
  {
    return std::tie(flags, ds_topo, ds_groups, coszen, hyd_stage, hyd_frost, hist_version, accum_version, irr_stage, wb_irrig, route_withdraw,
                    irr_supply, route_dam, route_heat, land, route_cmd, points_version, hyd_lat);
  }
  bool operator==(const StepKey& o) const { return tie() == o.tie(); }
};

struct GraphSlot {
  hipGraphExec_t exec = nullptr;
  double dt = 0.0;
  hipStream_t stream = nullptr;
  StepKey key;
  void drop()  // (nothing may still run it)
  {
    if (exec) (void)hipGraphExecDestroy(exec);
    exec = nullptr;
  }
};

}  // namespace elmk

using namespace elmk;  // (every unit that includes this header is written inside the library's namespace)

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
    // an entry over a feature row (elmk_column_history_add_row): its family, or -1; `field` then holds ELMK_RESTART_ROW_FIELD(family, which)
    int family = -1;
    // an entry over a cell row of the river stages (elmk_cell_history_add_row): `cells` is false, cld the routing's, the accumulators cld
    // doubles counted in elmk_device_bytes; family holds ELMK_ROWS_NFAMILY + the cell-row family and `field` its ELMK_RESTART_ROW_FIELD
    bool cellrow = false;
  };
  std::vector<HistEntry> hist;
  std::vector<HistRow> hist_rows;
  std::vector<HistRow> hist_crows;
  std::vector<HistRow> hist_rrows;  // the rows of cell-row entries, as the device table hist_rtable (allocated by the first such entry)
  DevBuf<HistRow> hist_table;
  DevBuf<HistRow> hist_rtable;
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
  // its frost-table extension (elmk_soil_hydrology_frost_*): the ELMK_HYDF_NROWS fp64 rows [row][ld], held while the extension is enabled
  DevBuf<double> hydf_rows;
  // its hillslope lateral flow (elmk_hillslope_*; api_hillslope.cpp): one allocation `mem` holds the ELMK_HS_NROWS fp64 rows [row][ld],
  // the geometry dist, width, area, elev [HS_NGEOM][ld], down [ld] (-2 in the padding columns), the uphill map [npad][ld] and the
  // budget's reduction partials [ELMK_CONS_NPART][3] and triple [3]; held exactly while the extension is on
  struct Hillslope {
    DevBuf<char> mem;
    double* rows = nullptr;
    double* geom = nullptr;
    int32_t* down = nullptr;
    int32_t* up = nullptr;
    double* part = nullptr;
    double* out = nullptr;
    int npad = 0;
    double k_aniso = 0.0;
  } hs;
  // water balance (elmk_water_balance_*): the ELMK_WB_NROWS fp64 rows [row][ld] and, in wb_red, the reduction's stage-1 partials
  // [3][ELMK_CONS_NPART][3], its triples [3][3] and the census {nbad, first bad column}; held exactly while the feature is enabled.
  // wb_ring: the run's ring rows, per buffer b and step the triples (wb_ring_mms: rows b * max_steps .., 9 doubles each) and the census
  // (wb_ring_census: 2 words each), held while the feature is enabled and a run is reserved.  wb_ran: the last elmk_run carried the flag;
  // wb_ran_empty: and enqueued no stage (the land unit)
  DevBuf<double> wb_rows;
  DevBuf<char> wb_red, wb_ring;
  double* wb_part = nullptr;
  double* wb_out = nullptr;
  long long* wb_census = nullptr;
  double* wb_ring_mms = nullptr;
  long long* wb_ring_census = nullptr;
  double wb_tol = 0.0;
  bool wb_ran = false, wb_ran_empty = false;
  // irrigation (elmk_irrigation_*): one allocation holds the three fp64 rows [row][ld] and behind them the int32 parameter row sched
  // [ld], held exactly while the feature is enabled
  DevBuf<double> irr_rows;
  int32_t* irr_sched = nullptr;
  // its river supply limit (elmk_irrigation_supply_*): the four fp64 cell rows [ELMK_IRRSUP_*][route.cld] and the threshold, held exactly
  // while the limit is on
  DevBuf<double> irrsup_rows;
  double irrsup_thr = 0.0;
  // The river stage (elmk_routing_*) has seven parts, each with one allocation held exactly while the part is on; api_routing.cpp's
  // table PARTS says the rest about each (rows, public ids, budget, restart rows, refusals).
  //   base (elmk_routing_enable): `mem` holds the rows [ROUTE_NROWS][cld], KOUT and area [cld], the upstream map [npad][cld], down
  //     [cld] and the budgets' reduction partials [3][ELMK_CONS_NPART][3] and triples [3][3].  ncalls: the calls since the last
  //     elmk_routing_init / _reset_mean (QOUT_SUM's count)
  //   kw (elmk_routing_kinematic_*): the scheme's rows [KW_NROWS][cld]; tab: the derived parameters [KW_NPAR][cld]
  //   fp (elmk_routing_inundation_*): the floodplain's rows [FP_NROWS][cld]; tab: the host's tables [FP_NTAB][cld]
  //   dam (elmk_routing_reservoir_*): the reservoirs' rows [DAM_NROWS][cld]; tab: the host's tables [DAM_NTAB][cld]; beside it, in
  //     the same allocation, MSTART [cld].  dam_time: the month | begins << 4 of elmk_routing_reservoir_time, what the stepwise calls read
  //   heat (elmk_routing_heat_*): the stream temperature's rows [HT_NROWS][cld]; tab: KSW [cld].  heat_sublev: the soil layer of H1
  //   land (elmk_floodplain_infiltration_*): the cell row QLAND [1][cld]; tab: the three column rows [ELMK_FPI_NROWS][ld]; beside them, in
  //     the same allocation, cellof [ld] (land_cellof; -1 in the padding columns)
  //   cmd (elmk_routing_command_*): the command areas' rows [CMD_NROWS][cld]; tab: share and claim [2][CMD_NDEP][cld]; beside them, in
  //     the same allocation, a row of 1.0 [cld] (what RATIO is reset from), the cells' dam row [CMD_NDEP][cld] (cmd_dam) and the inverse
  //     map: cmd_dams [cmd_ndams], cmd_ptr [cmd_ndams + 1], cmd_tcell and cmd_tshare [terms]
  // route_launch takes the scheme and the forms whose memory is there.
  struct Routing {
    struct Part {
      DevBuf<char> mem;
      double* rows = nullptr;
      double* tab = nullptr;
    };
    DevBuf<char> mem;
    int64_t ncells = 0, cld = 0;
    int npad = 0, nsub = 0;
    bool withdraw = false;
    int64_t ncalls = 0;
    double* rows = nullptr;
    double* kout = nullptr;
    double* area = nullptr;
    int32_t* up = nullptr;
    int32_t* down = nullptr;
    double* part = nullptr;
    double* out = nullptr;
    Part kw, fp, dam, heat, land, cmd;
    double *cmd_ones = nullptr, *cmd_tshare = nullptr;
    int32_t *cmd_dam = nullptr, *cmd_dams = nullptr, *cmd_tcell = nullptr;
    int64_t* cmd_ptr = nullptr;
    int64_t cmd_ndams = 0;
    int32_t* land_cellof = nullptr;
    int32_t* dam_mstart = nullptr;
    int32_t dam_time = 0;
    int heat_sublev = 0;
  } route;
  bool restart_cells = false;  // ELMK_OPT_RESTART_CELLS: the image carries the routing state (version 6)
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
  // point series (elmk_points_*; api_points.cpp): the entries and the two lists as the host holds them; `mem` holds the device table
  // k_points_record reads, the run's base word and the two lists [ELMK_POINTS_MAX_POINTS] each; `ring` the records [max_records][stride],
  // stride = POINTS_HEAD + the entries' points, each entry padded to 8 doubles; `stamps` the decday of every row of the run's two step
  // tables (with its pinned host copy, allocated by the first armed elmk_run of a reservation).  total: the records since the last
  // reset, known on the host when a record is enqueued.  version: counts every change of what a captured run step holds of the part;
  // the step's key takes it while the part is armed (run_on) and 0 otherwise.
  struct Points {
    struct Entry {
      int kind, a, b;  // POINTS_* of api_points.cpp and the source's two ids (field, level; family, which)
      const void* src;
      int dtype;
    };
    std::vector<Entry> entries;
    std::vector<int64_t> list[ELMK_POINTS_NKIND];
    DevBuf<char> mem;
    PointsTable* table = nullptr;
    int32_t* base = nullptr;
    int64_t* dlist[ELMK_POINTS_NKIND] = {};
    DevBuf<double> ring;
    int max_records = 0;
    int64_t stride = 0;
    int nwaves = 0;
    DevBuf<double> stamps;
    DevBuf<double, true> stamps_host;
    int stamps_steps = 0;
    int64_t total = 0;
    bool run_on = false;
    uint64_t version = 0;
  } pts;
  std::string err;
};

namespace elmk {

// ---- errors and entry (elmk_api.cpp) ----
bool hip_fail(elmk_ctx* ctx, hipError_t e, const char* what);

#define HIPCHK(call)                                      \
  do {                                                    \
    if (hip_fail(ctx, (call), #call)) return ELMK_E_HIP;  \
  } while (0)

int invalid(elmk_ctx* ctx, const char* msg);
int launched(elmk_ctx* ctx);  // how an entry point that only launches ends: the launches' error, if any
int synced(elmk_ctx* ctx);    // ... and one that waits for the context's stream
// a refusal of elmk_maps.h's checks (text, or nullptr for none) under the entry point's name
int invalid_map(elmk_ctx* ctx, const char* who, const char* text);
// "<who>: bad column range" unless [col0, col0 + n) lies in 0 .. lim and host is there to take n > 0 values
int check_range(elmk_ctx* ctx, const char* who, const void* host, int64_t col0, int64_t n, int64_t lim, const char* what = "column");
int enter(elmk_ctx* ctx);
int enter_physics(elmk_ctx* ctx);  // what every physics entry point does before it launches
int push_params(elmk_ctx* ctx);
int heal_lists(elmk_ctx* ctx);
// the calls that allocate, free or wait cannot be part of a caller's captured graph: "<who>: the stream is being captured"
int refuse_capture(elmk_ctx* ctx, const char* who);
int quiesce(elmk_ctx* ctx, bool uploads);
int drop_graphs(elmk_ctx* ctx);
int set_col_dayl(elmk_ctx* ctx, bool on);
int xfer_rows(elmk_ctx* ctx, char* dev, int64_t ld, int es, int nlev, void* host, int64_t col0, int64_t n, int layout, bool up);

// never write under a run that reads it: wait for the end of every enqueued, unfinished run whose buffer b `reads` selects
template <class Pred>
int wait_for_runs(elmk_ctx* ctx, Pred reads)
{
  for (int b = 0; b < 2; b++)
    if (ctx->run.live[b] && reads(b)) HIPCHK(hipEventSynchronize(ctx->run_done[b]));
  return ELMK_OK;
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

// ---- stage lists (elmk_api.cpp) ----
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

void launch_advance(elmk_ctx* ctx, double dt);  // every stage of elmk_advance_physics, as one stage of the run step
int enqueue_stages(elmk_ctx* ctx, Stages L, double dt, hipEvent_t* marks = nullptr, bool per_stage = true);
// a sequence elmk_set_graph applies to: replayed from its captured graph, or enqueued stage by stage
int launch_sequence(elmk_ctx* ctx, GraphId id, Stages L, double dt, const StepKey& key = StepKey{});

// ---- what the run step and the restart images need of the features ----
unsigned long long* hist_counts(elmk_ctx* ctx);  // api_history.cpp
unsigned hist_tape_mask(const elmk_ctx* ctx);
void mark_sampled(elmk_ctx* ctx, unsigned mask);
void hist_accumulate_launch(elmk_ctx* ctx);
unsigned long long* accum_counts(elmk_ctx* ctx);  // api_accum.cpp
void accum_update_launch(elmk_ctx* ctx);
// a feature that keeps fp64 rows [row][ld] of its own beside the state (api_rows.cpp, api_irrigation.cpp)
struct Rows {
  DevBuf<double> elmk_ctx::*buf;
  int nrows;
  const char* label;   // in the text of a HIP error
  const char* enable;  // the enabling call, for refusals
  int family;          // ELMK_ROWS_*: history entries over these rows (elmk_column_history_add_row) bar the clear
};
extern const Rows ROWS_OF_IRRIGATION;  // api_irrigation.cpp
int rows_held(elmk_ctx* ctx, const Rows& R, const char* who);   // refuses while a history entry reads the family's rows
int rows_enter(elmk_ctx* ctx, const Rows& R, const char* who);  // how every call but enable and clear begins
int rows_read(elmk_ctx* ctx, const Rows& R, const char* who, int which, double* host, int64_t col0, int64_t n);
int rows_clear(elmk_ctx* ctx, const Rows& R, const char* who);
constexpr int IRR_NROWS = 3;
void irr_run_launch(elmk_ctx* ctx, double dt);  // the run step's irrigation stage (api_irrigation.cpp)
// "<who>: the irrigation's river supply limit is on (elmk_irrigation_supply_clear first)" while it is - what the limit reads stays
int irrsup_holds(elmk_ctx* ctx, const char* who);
void route_launch(elmk_ctx* ctx, double dt, bool run = false);  // one call of the runoff routing (api_routing.cpp); run: inside elmk_run's step
// "<who>: runoff routing is enabled (elmk_routing_clear first)" while it is - what the routing reads stays; with_withdrawal: only while
// the withdrawal is on
int route_holds(elmk_ctx* ctx, const char* who, bool with_withdrawal = false);
// "<who>: the floodplain infiltration is on (elmk_floodplain_infiltration_clear first)" while it is - what its kernels' forms read stays
int land_holds(elmk_ctx* ctx, const char* who);
// row `which` (ELMK_ROUTE_*) of the river stages as elmk_routing_read finds it now, or null with *why set (not enabled, out of range, its
// scheme or extension off)
const double* route_row(const elmk_ctx* ctx, int which, const char** why);
size_t route_bytes(const elmk_ctx* ctx);  // the device bytes of the parts that are on
int route_zero_rows(elmk_ctx* ctx);       // every row of every part that is on zero (enqueued)
// the routing state of the restart image (ELMK_OPT_RESTART_CELLS): the ELMK_ROUTE_* of the prognostic rows the parts hold at this
// moment, in image order (VOLR, QOUT_SUM, WH, WT, WF, RES, KRLS, or TT, TR behind WT: the heat excludes the two before it; with the
// floodplain infiltration on FLOOD_FRAC, which its F1 reads before the next call rewrites it, comes last); returns their number
constexpr int ROUTE_STATE_MAX = 8;
int route_state_rows(const elmk_ctx* ctx, int* ids);
constexpr int ALT_NROWS = 3;  // api_rows.cpp
ActiveLayerArgs alt_args(const elmk_ctx* ctx);
bool hyd_land(const elmk_ctx* ctx);
void hyd_launch(elmk_ctx* ctx, double dt);
// the hillslope lateral flow (api_hillslope.cpp): "<who>: the hillslope lateral flow is on (elmk_hillslope_clear first)" while it is;
// "<who>: history entries over the hillslope rows exist (elmk_history_clear first)" or the point series' text while an entry reads its
// rows; the release (the stream is idle)
int hs_excludes(elmk_ctx* ctx, const char* who);
int hs_held(elmk_ctx* ctx, const char* who);
void hs_release(elmk_ctx* ctx);
int wb_ring_alloc(elmk_ctx* ctx);  // the water balance's ring rows of the current reservation, if the feature is enabled (the stream is idle)
void wb_begin_launch(elmk_ctx* ctx);
void wb_launch(elmk_ctx* ctx, double dt, bool run);
// the rows of a feature family (ELMK_ROWS_*) for a history entry: the device row `which`, or null with *why set (unknown family, not
// enabled, which out of range)
const double* feature_row(const elmk_ctx* ctx, int family, int which, const char** why);
int hist_has_family(const elmk_ctx* ctx, int family);  // a row entry of the family exists (api_history.cpp)
// "<who>: cell-row history entries exist on its rows (elmk_history_clear first)" while an entry of elmk_cell_history_add_row samples row
// which0 .. which1 of the cell-row family (family < 0: any family, any row)
int cellrows_hold(elmk_ctx* ctx, const char* who, int family = -1, int which0 = 0, int which1 = 0);
// the rows of a cell-row family (ELMK_CELL_ROWS_*) for a history or point-series entry: the device row `which` over the routing's cells, or
// null with *why set - exactly the rows elmk_routing_read / elmk_irrigation_supply_read accept at this moment (api_history.cpp)
const double* cell_row(const elmk_ctx* ctx, int family, int which, const char** why);
// point series (api_points.cpp).  The interlocks of P7, each "<who>: point-series entries ... (elmk_points_clear first)": an entry over
// the rows of a feature family; an entry over row which0 .. which1 of a cell-row family (family < 0: any cell-row entry); a gridded or
// cell-row entry or a cells list, which hold the output grid's map and its ncells
int points_hold_family(elmk_ctx* ctx, const char* who, int family);
int points_hold_cellrows(elmk_ctx* ctx, const char* who, int family, int which0, int which1);
int points_hold_grid(elmk_ctx* ctx, const char* who);
// elmk_run with the part armed: the refusals (before anything is enqueued), then the stamps and the base word of the run on buffer buf,
// enqueued; the run step's stage; the armed part's key
int points_run_check(elmk_ctx* ctx);
int points_run_begin(elmk_ctx* ctx, int buf, const elmk_run_step* steps, int nsteps);
void points_run_launch(elmk_ctx* ctx);
inline uint64_t points_key(const elmk_ctx* ctx) { return ctx->pts.run_on ? ctx->pts.version : 0; }
// downscaling TOPO mode: the forcing kernels' parameters (ds_topo false: OFF, the kernels as they were); api_run.cpp
inline bool ds_topo(const elmk_ctx* ctx) { return ctx->ds.mode == ELMK_DS_TOPO; }
DsParams ds_params(const elmk_ctx* ctx);
void ds_lw_norm(elmk_ctx* ctx);
int sw_reset(elmk_ctx* ctx, int mode, double forc_dt);  // shortwave: set the mode and forget every record time

}  // namespace elmk
