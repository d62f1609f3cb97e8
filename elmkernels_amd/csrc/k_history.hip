// k_history.hip - history accumulation on the device (elmk_history_*): running sums, extremes and last values of registered state
// fields, folded in once per step by ONE launch, so a driver downloads a time average once per output interval instead of the
// state after every step.
//
// The unit of work is a row: one level of one registered entry (HistRow, built on the host by elmk_history_add).  The grid is
// column blocks x rows, so the op and the stored dtype are uniform across a workgroup (no divergence) and every access is a
// coalesced SoA stream over the columns of one row.  Every thread takes two adjacent columns: a 16-byte load / store of the fp64
// accumulator and an 8-, 4- or 2-byte load of the source.  Rows of state fields and accumulators start at multiples of the level
// stride ld (a multiple of 64 columns) from 256-byte aligned bases, so the vector accesses are aligned, and ncols <= ld keeps the
// second column of a pair inside the row.  Bytes per column and row: source element + 16 (accumulator read + write).
//
// Semantics (include/elmk.h, "history"): each sample is the stored value widened to fp64; SUM / AVG acc = acc + v from -0.0;
// MAX acc = (v > acc || v != v) ? v : acc from -inf (a NaN sticks), MIN the mirror from +inf; INST acc = v.  AVG is divided by
// the count when it is read (k_hist_finalize), one correctly rounded division.
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_pair.h"

// Every source load and every accumulator load and store carries the nontemporal hint: interleaved A/B runs of
// tests/tools/history_cost.py --ab (profiles/r06_history_nt_ab.jsonl) took the 19-field PrimaryVars tape from 0.64 to 0.59 ms at
// 1 M columns and from 6.25 to 5.84 ms at 10 M, the 12-flux tape from 0.49 to 0.46 ms at 10 M.  Only a tape small enough to stay
// in the on-die caches between two launches back to back lost (12 fluxes at 1 M: 0.039 -> 0.046 ms), and a physics step between
// two accumulates leaves nothing of it there.

namespace elmk {

namespace {
// one column of a source row, widened to fp64 as load_pair widens it (a gather: no nontemporal hint, neighbouring cells re-read lines)
__device__ __forceinline__ double load_one(const void* src, int dtype, int64_t c)
{
  switch (dtype) {
    case ELMK_F64: return ((const ELMK_GLOBAL double*)src)[c];
    case ELMK_F32_STORED: return (double)((const ELMK_GLOBAL float*)src)[c];
    case ELMK_I32: return (double)((const ELMK_GLOBAL int32_t*)src)[c];
    case ELMK_U32: return (double)((const ELMK_GLOBAL uint32_t*)src)[c];
    default: return (double)((const ELMK_GLOBAL uint8_t*)src)[c];
  }
}

__device__ __forceinline__ double fold(int op, double acc, double v)
{
  switch (op) {
    case ELMK_HIST_AVG:
    case ELMK_HIST_SUM: return acc + v;
    case ELMK_HIST_MAX: return (v > acc || v != v) ? v : acc;
    case ELMK_HIST_MIN: return (v < acc || v != v) ? v : acc;
    default: return v;  // ELMK_HIST_INST
  }
}
// column pair p of a column row
__device__ __forceinline__ void fold_pair(const HistRow& r, int64_t p)
{
  const int64_t c = 2 * p;
  const hd2 v = load_pair(r.src, r.dtype, c);
  ELMK_GLOBAL hd2* a = (ELMK_GLOBAL hd2*)r.acc + p;
  hd2 acc = h_ld(a);
  acc.x = fold(r.op, acc.x, v.x);
  acc.y = fold(r.op, acc.y, v.y);
  h_st(a, acc);
}
}  // namespace

// grid (column pairs / 256, rows); rows[blockIdx.y] is uniform across the workgroup
__global__ __launch_bounds__(256) void k_hist_accumulate(const HistRow* __restrict__ rows, unsigned long long* __restrict__ counts,
                                                         int64_t npairs, unsigned tape_mask)
{
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++)
      if (tape_mask & (1u << t)) atomicAdd(&counts[t], 1ull);
  }
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const HistRow r = rows[blockIdx.y];
  fold_pair(r, p);
}

// the rows of one tape back to their initial value, the tape's count to 0 (rows of other tapes: nothing)
__global__ __launch_bounds__(256) void k_hist_reset(const HistRow* __restrict__ rows, int nrows, unsigned long long* __restrict__ counts,
                                                    int64_t npairs, int tape)
{
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counts[tape] = 0ull;
  if ((int)blockIdx.y >= nrows) return;
  const HistRow r = rows[blockIdx.y];
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r.tape != tape || p >= npairs) return;
  const double v = hist_init_value(r.op);
  ((ELMK_GLOBAL hd2*)r.acc)[p] = hd2{v, v};
}

// result of one entry for columns [col0, col0 + m): acc / count for AVG, acc otherwise, into out[lev * m + i] (dense SoA)
__global__ __launch_bounds__(256) void k_hist_finalize(const double* __restrict__ acc, int64_t ld, int op, int64_t count, int64_t col0,
                                                       int64_t m, double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int lev = blockIdx.y;
  const double a = acc[(int64_t)lev * ld + col0 + i];
  out[(int64_t)lev * m + i] = op == ELMK_HIST_AVG ? a / (double)count : a;
}

static unsigned pair_blocks(int64_t npairs) { return (unsigned)(npairs > 0 ? (npairs + 255) / 256 : 1); }

void launch_hist_accumulate(const HistRow* rows, int nrows, unsigned long long* counts, int64_t ncols, unsigned tape_mask,
                            hipStream_t st)
{
  if (nrows <= 0) return;
  const int64_t npairs = (ncols + 1) / 2;
  hipLaunchKernelGGL(k_hist_accumulate, dim3(pair_blocks(npairs), (unsigned)nrows), dim3(256), 0, st, rows, counts, npairs, tape_mask);
}

void launch_hist_reset(const HistRow* rows, int nrows, unsigned long long* counts, int64_t ncols, int tape, hipStream_t st)
{
  const int64_t npairs = (ncols + 1) / 2;
  hipLaunchKernelGGL(k_hist_reset, dim3(pair_blocks(npairs), (unsigned)(nrows > 0 ? nrows : 1)), dim3(256), 0, st, rows, nrows, counts,
                     npairs, tape);
}

void launch_hist_finalize(const double* acc, int64_t ld, int nlev, int op, int64_t count, int64_t col0, int64_t m, double* out,
                          hipStream_t st)
{
  if (m <= 0) return;
  hipLaunchKernelGGL(k_hist_finalize, dim3((unsigned)((m + 255) / 256), (unsigned)nlev), dim3(256), 0, st, acc, ld, op, count, col0, m,
                     out);
}

// ---------------------------------------------------------------------------------------------------
// output grid (elmk_set_output_grid, elmk_download_gridded, elmk_gridded_history_add): columns averaged onto cells through a CSR map.
// The value of cell i of a source row x is w[p0] * x[col[p0]], then + w[p] * x[col[p]] for p = p0+1 .. p1-1 in that order, with no
// contraction; a cell with no terms is `fill`.  One workgroup takes AGG_CELLS consecutive cells of one row, and the terms of those
// cells are one contiguous span of the map: the workgroup walks it in tiles of AGG_TILE terms, every thread forming the products of
// its share of a tile with coalesced loads of col and w (and of x, when a cell's columns are contiguous) into LDS, then thread t
// adds the products of cell t out of LDS in CSR order.  A product is one rounding whichever lane forms it, and every sum is taken
// by one lane in term order, so the result is the host's (regrid.apply_aggregate) bit for bit; no atomics.
// ---------------------------------------------------------------------------------------------------
namespace {
constexpr int AGG_THREADS = 256, AGG_CELLS = 64, AGG_TILE = 2048;

// cells [c0, min(c0 + CELLS, cend)) of the source row src; called by every thread of the workgroup (it has barriers, and c0 is
// uniform).  Thread t < CELLS returns the value of cell c0 + t (fill for an empty cell or a thread past the end) and in *empty
// whether that cell has no terms.
template <int CELLS = AGG_CELLS>
__device__ __forceinline__ double agg_cells(const void* src, int dtype, const OGridMap& M, int64_t c0, int64_t cend, double* tile,
                                            bool* empty)
{
  const int t = threadIdx.x;
  const int64_t c1 = c0 + CELLS < cend ? c0 + CELLS : cend;
  const int64_t P0 = M.ptr[c0], P1 = M.ptr[c1];
  int64_t p0 = 0, p1 = 0;
  if (t < CELLS && c0 + t < c1) {
    p0 = M.ptr[c0 + t];
    p1 = M.ptr[c0 + t + 1];
  }
  double v = M.fill;
  for (int64_t base = P0; base < P1; base += AGG_TILE) {
    const int m = (int)(P1 - base < AGG_TILE ? P1 - base : AGG_TILE);
#pragma unroll
    for (int k = 0; k < AGG_TILE / AGG_THREADS; k++) {
      const int q = k * AGG_THREADS + t;
      if (q < m) tile[q] = M.w[base + q] * load_one(src, dtype, M.col[base + q]);
    }
    __syncthreads();
    const int64_t lo = p0 > base ? p0 : base, hi = p1 < base + m ? p1 : base + m;
    for (int64_t p = lo; p < hi; p++) {
      const double x = tile[p - base];
      v = p == p0 ? x : v + x;
    }
    __syncthreads();
  }
  *empty = p0 == p1;
  return v;
}
}  // namespace

// cells [cell0, cell0 + m) of one source row into out[0 .. m); grid (ceil(m / AGG_CELLS))
__global__ __launch_bounds__(AGG_THREADS) void k_ogrid_aggregate(const void* __restrict__ src, int dtype, OGridMap M, int64_t cell0,
                                                                 int64_t m, double* __restrict__ out)
{
  __shared__ double tile[AGG_TILE];
  const int64_t c0 = cell0 + (int64_t)blockIdx.x * AGG_CELLS;
  bool empty;
  const double v = agg_cells(src, dtype, M, c0, cell0 + m, tile, &empty);
  if (threadIdx.x < AGG_CELLS && c0 + threadIdx.x < cell0 + m) out[c0 - cell0 + threadIdx.x] = v;
}

// k_hist_accumulate with cell rows after the column rows: grid (max(column pair blocks, cell blocks), nrows + ncrows).  Row y < nrows
// is a column row, folded as k_hist_accumulate folds it; row nrows + k is cell row crows[k]: acc[c] = fold(op, acc[c], aggregate of
// cell c of the current value), skipped for an empty cell (it reads fill).
__global__ __launch_bounds__(256) void k_hist_accumulate_cells(const HistRow* __restrict__ rows, int nrows, const HistRow* __restrict__ crows,
                                                               OGridMap M, unsigned long long* __restrict__ counts, int64_t npairs,
                                                               unsigned tape_mask)
{
  static_assert(AGG_THREADS == 256, "one block shape for both kinds of rows");
  __shared__ double tile[AGG_TILE];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++)
      if (tape_mask & (1u << t)) atomicAdd(&counts[t], 1ull);
  }
  if ((int)blockIdx.y < nrows) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npairs) return;
    const HistRow r = rows[blockIdx.y];
    fold_pair(r, p);
    return;
  }
  const int64_t c0 = (int64_t)blockIdx.x * AGG_CELLS;
  if (c0 >= M.ncells) return;
  const HistRow r = crows[blockIdx.y - nrows];
  bool empty;
  const double g = agg_cells(r.src, r.dtype, M, c0, M.ncells, tile, &empty);
  const int64_t c = c0 + threadIdx.x;
  if (threadIdx.x < AGG_CELLS && c < M.ncells && !empty) r.acc[c] = fold(r.op, r.acc[c], g);
}

// k_hist_accumulate_cells with the rows of cell-row entries (elmk_cell_history_add_row) after the gridded rows: grid (max(column pair
// blocks, gridded cell blocks, cell pair blocks), nrows + ncrows + the cell-row count).  Row nrows + ncrows + k is rrows[k]: a fp64 row
// over the output grid's cells that is its own sample - no map, no fill, every cell a sample - folded by pairs as a column row is: the
// rows and their accumulators start 256-byte aligned and span cld cells, a multiple of 64, so the second cell of a pair stays inside.
// Launched only while such an entry exists; the two kernels above are what every other context runs.
__global__ __launch_bounds__(256) void k_hist_accumulate_rows(const HistRow* __restrict__ rows, int nrows, const HistRow* __restrict__ crows,
                                                              int ncrows, const HistRow* __restrict__ rrows, OGridMap M,
                                                              unsigned long long* __restrict__ counts, int64_t npairs, int64_t rpairs,
                                                              unsigned tape_mask)
{
  __shared__ double tile[AGG_TILE];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    for (int t = 0; t < ELMK_HIST_MAX_TAPES; t++)
      if (tape_mask & (1u << t)) atomicAdd(&counts[t], 1ull);
  }
  const int y = (int)blockIdx.y;
  if (y < nrows || y >= nrows + ncrows) {
    const bool cellrow = y >= nrows;
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (cellrow ? rpairs : npairs)) return;
    const HistRow r = cellrow ? rrows[y - nrows - ncrows] : rows[y];
    fold_pair(r, p);
    return;
  }
  const int64_t c0 = (int64_t)blockIdx.x * AGG_CELLS;
  if (c0 >= M.ncells) return;
  const HistRow r = crows[y - nrows];
  bool empty;
  const double g = agg_cells(r.src, r.dtype, M, c0, M.ncells, tile, &empty);
  const int64_t c = c0 + threadIdx.x;
  if (threadIdx.x < AGG_CELLS && c < M.ncells && !empty) r.acc[c] = fold(r.op, r.acc[c], g);
}

// cells [cell0, cell0 + m) of one gridded entry's result into out[lev * m + i]: fill for an empty cell, else as k_hist_finalize
__global__ __launch_bounds__(256) void k_ogrid_finalize(const double* __restrict__ acc, int64_t ld, int op, int64_t count,
                                                        const int64_t* __restrict__ ptr, double fill, int64_t cell0, int64_t m,
                                                        double* __restrict__ out)
{
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int lev = blockIdx.y;
  const int64_t c = cell0 + i;
  const double a = acc[(int64_t)lev * ld + c];
  out[(int64_t)lev * m + i] = ptr[c] == ptr[c + 1] ? fill : op == ELMK_HIST_AVG ? a / (double)count : a;
}

static unsigned cell_blocks(int64_t ncells) { return (unsigned)(ncells > 0 ? (ncells + AGG_CELLS - 1) / AGG_CELLS : 1); }

// downscaling's longwave renormalisation (elmk_set_downscaling_groups; ELM's downscale_longwave): the groups are an output-grid map
// (fill 0, a column in at most one group), so agg_cells gives each group's A = sum w * Lg and S = sum w * Lc in term order.  Then, for
// the cells of this workgroup, norm = (W == 0 || A == 0) ? 1 : (A / W) / (S / W), and every thread scales its share of the span's
// terms: term q belongs to the cell k with ptr[c0 + k] <= q < ptr[c0 + k + 1] (a search over the span's ptr in LDS).  A column is
// read and written only by the workgroup of its one group, after that workgroup's sums, so one launch needs no atomics.  A gridcell
// holds far more columns than an output cell holds terms on average, so a workgroup takes DS_CELLS groups, not AGG_CELLS: at 1 M
// columns in groups of 150 that is 417 workgroups instead of 105, and each lane's serial sum is the only long chain left.
constexpr int DS_CELLS = 16;
__global__ __launch_bounds__(AGG_THREADS) void k_ds_lw_norm(void* __restrict__ lw, int lw_dtype, const double* __restrict__ lg, OGridMap M,
                                                            const double* __restrict__ wsum)
{
  __shared__ double tile[AGG_TILE];
  __shared__ double norm[DS_CELLS];
  __shared__ int64_t sp[DS_CELLS + 1];
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * DS_CELLS;
  const int64_t c1 = c0 + DS_CELLS < M.ncells ? c0 + DS_CELLS : M.ncells;
  bool empty;
  const double A = agg_cells<DS_CELLS>(lg, ELMK_F64, M, c0, M.ncells, tile, &empty);
  const double S = agg_cells<DS_CELLS>(lw, lw_dtype, M, c0, M.ncells, tile, &empty);
  if (t < DS_CELLS && c0 + t < c1) {
    const double W = wsum[c0 + t];
    norm[t] = (W == 0.0 || A == 0.0) ? 1.0 : (A / W) / (S / W);
  }
  if (t <= DS_CELLS && c0 + t <= c1) sp[t] = M.ptr[c0 + t];
  __syncthreads();
  const int ncl = (int)(c1 - c0);
  for (int64_t q = sp[0] + t; q < sp[ncl]; q += AGG_THREADS) {
    int lo = 0, hi = ncl;  // sp[lo] <= q < sp[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sp[mid] <= q) lo = mid;
      else hi = mid;
    }
    const int64_t c = M.col[q];
    if (lw_dtype == ELMK_F64) {
      ELMK_GLOBAL double* p = (ELMK_GLOBAL double*)lw + c;
      *p = *p * norm[lo];
    } else {  // ELMK_F32_STORED: widened, scaled in fp64, rounded on store
      ELMK_GLOBAL float* p = (ELMK_GLOBAL float*)lw + c;
      *p = (float)((double)*p * norm[lo]);
    }
  }
}

void launch_ds_lw_norm(void* lw, int lw_dtype, const double* lg, const OGridMap& M, const double* wsum, hipStream_t st)
{
  if (M.ncells <= 0) return;
  hipLaunchKernelGGL(k_ds_lw_norm, dim3((unsigned)((M.ncells + DS_CELLS - 1) / DS_CELLS)), dim3(AGG_THREADS), 0, st, lw, lw_dtype, lg, M, wsum);
}

void launch_ogrid_aggregate(const void* src, int dtype, const OGridMap& M, int64_t cell0, int64_t m, double* out, hipStream_t st)
{
  if (m <= 0) return;
  hipLaunchKernelGGL(k_ogrid_aggregate, dim3(cell_blocks(m)), dim3(AGG_THREADS), 0, st, src, dtype, M, cell0, m, out);
}

void launch_hist_accumulate_cells(const HistRow* rows, int nrows, const HistRow* crows, int ncrows, const OGridMap& M,
                                  unsigned long long* counts, int64_t ncols, unsigned tape_mask, hipStream_t st)
{
  const int64_t npairs = (ncols + 1) / 2;
  const unsigned pb = nrows > 0 ? pair_blocks(npairs) : 1u, cb = cell_blocks(M.ncells);
  const unsigned bx = pb > cb ? pb : cb;
  hipLaunchKernelGGL(k_hist_accumulate_cells, dim3(bx, (unsigned)(nrows + ncrows)), dim3(256), 0, st, rows, nrows, crows, M, counts, npairs,
                     tape_mask);
}

void launch_hist_accumulate_rows(const HistRow* rows, int nrows, const HistRow* crows, int ncrows, const HistRow* rrows, int nrrows,
                                 const OGridMap& M, unsigned long long* counts, int64_t ncols, unsigned tape_mask, hipStream_t st)
{
  if (nrrows <= 0) return;
  const int64_t npairs = (ncols + 1) / 2, rpairs = (M.ncells + 1) / 2;
  const unsigned pb = nrows > 0 ? pair_blocks(npairs) : 1u, cb = ncrows > 0 ? cell_blocks(M.ncells) : 1u, rb = pair_blocks(rpairs);
  const unsigned pc = pb > cb ? pb : cb, bx = pc > rb ? pc : rb;
  hipLaunchKernelGGL(k_hist_accumulate_rows, dim3(bx, (unsigned)(nrows + ncrows + nrrows)), dim3(256), 0, st, rows, nrows, crows, ncrows, rrows,
                     M, counts, npairs, rpairs, tape_mask);
}

void launch_ogrid_finalize(const double* acc, int64_t ld, int nlev, int op, int64_t count, const int64_t* ptr, double fill, int64_t cell0,
                           int64_t m, double* out, hipStream_t st)
{
  if (m <= 0) return;
  hipLaunchKernelGGL(k_ogrid_finalize, dim3((unsigned)((m + 255) / 256), (unsigned)nlev), dim3(256), 0, st, acc, ld, op, count, ptr, fill,
                     cell0, m, out);
}


// ---------------------------------------------------------------------------------------------------
// the irrigation's river supply limit (elmk_irrigation_supply_*; include/elmk.h "irrigation: river supply limit"): CLM5's
// limit_irrigation_if_rof_enabled / CalcDeficitVolrLimited at the daily demand check.  One launch right after k_irrigation on the same
// stream.  elmkernels_amd/irrigation.py: supply_limit() restates S0 - S6 in numpy, and the kernel follows them statement by statement:
// no contraction, plain IEEE comparisons, `/` the correctly rounded fp64 division; a NaN is stored into a row as the canonical quiet NaN.
//
// The shape is k_ds_lw_norm's: one workgroup takes SUP_CELLS consecutive cells of the output grid's map, whose terms are one contiguous
// span of the map.  The workgroup walks the span in tiles of SUP_TILE terms; every thread forms the two products of S2 of its share of a
// tile - coalesced loads of col and w, gathers of RATE, NLEFT and QFLX_IRRIG that are coalesced where a cell's columns are neighbours - into two LDS
// tiles, then thread t adds the products of cell t out of LDS in CSR order.  A product is one rounding whichever lane forms it and every
// sum is taken by one lane in term order, so D and C are regrid.apply_aggregate's bit for bit.  Both sums come from ONE walk of its own:
// agg_cells forms one sum per walk from a source row, and two walks would load the map and the rows twice; agg_cells and the kernels
// above are left exactly as they were.  Then S3, S4 and S6 per cell, and S5 only in a workgroup that has a cell with ratio != 1.0: every
// thread scales the checking columns of its share of the span, finding a term's cell by a binary search over the span's ptr in LDS.  A
// column is in at most one cell (checked when the limit is enabled), so it is read and written by one workgroup only, after that
// workgroup's sums: no atomics and no fence.
//
// SUP_CELLS = 64, as AGG_CELLS and not DS_CELLS: the map is the output grid's, whose cells hold few columns (four per cell fill the 256
// threads of a tile pass with one term each, and the 64 serial sums are four terms long), where a downscaling group holds a gridcell's
// 150.  SUP_TILE = 1024: two tiles of 8 KiB are k_ds_lw_norm's 16 KiB of LDS.  A quiet step - no column checking - reads col, w, RATE,
// NLEFT and QFLX_IRRIG once and writes three cell rows.  No nontemporal hint: none has been measured for it.
// ---------------------------------------------------------------------------------------------------
namespace {
constexpr int SUP_THREADS = AGG_THREADS, SUP_CELLS = 64, SUP_TILE = 1024;
static_assert(SUP_CELLS < SUP_THREADS && SUP_TILE % SUP_THREADS == 0, "thread t <= SUP_CELLS loads ptr; whole passes over a tile");

__device__ __forceinline__ void sup_st(gptr<double> p, double v)
{
  if (v != v) v = __builtin_nan("");
  *p = v;
}
}  // namespace

// D7 (include/elmk.h "reservoirs"): while the reservoirs are on, a dam cell's storage above SMIN counts as available beside the channel's
template <bool DAM>
struct SupDam {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct SupDam<true> {
  gptr<const double> res, smin, cap;  // [cld] each
};

// C6 (include/elmk.h "command areas"): while the command areas are on too, a cell's claims on the usable storage of the dams that
// supply it count as available as well; dam and claim are the cells' ELL rows [CMD_NDEP][cld]
template <bool CMD>
struct SupCmd {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct SupCmd<true> {
  gptr<const int32_t> dam;
  gptr<const double> claim;
};

// grid (ceil(ncells / SUP_CELLS)); irr = the irrigation's rows [3][ld], sup = the limit's rows [4][cld]
template <bool DAM = false, bool CMD = false>
__global__ __launch_bounds__(SUP_THREADS) void k_irrigation_supply(gptr<double> irr, int64_t ld, int idt, int nspd, OGridMap M,
                                                                   gptr<const double> area, gptr<const double> volr, double thr,
                                                                   gptr<double> sup, int64_t cld, SupDam<DAM> dm, SupCmd<CMD> cm)
{
  static_assert(!CMD || DAM, "the command areas need the reservoirs");
  __shared__ double tile_d[SUP_TILE];
  __shared__ double tile_c[SUP_TILE];
  __shared__ double ratio_s[SUP_CELLS];
  __shared__ int64_t sp[SUP_CELLS + 1];
  __shared__ int limited;
  const int t = threadIdx.x;
  const int64_t c0 = (int64_t)blockIdx.x * SUP_CELLS;
  const int64_t c1 = c0 + SUP_CELLS < M.ncells ? c0 + SUP_CELLS : M.ncells;
  const int ncl = (int)(c1 - c0);
  const gptr<double> rate = irr + (int64_t)ELMK_IRR_RATE * ld;
  const gptr<const double> nleft = irr + (int64_t)ELMK_IRR_NLEFT * ld, qirr = irr + (int64_t)ELMK_IRR_QFLX_IRRIG * ld;
  const double dnspd = (double)nspd, didt = (double)idt;

  if (t == 0) limited = 0;
  if (t <= ncl) sp[t] = M.ptr[c0 + t];
  __syncthreads();
  const int64_t P0 = sp[0], P1 = sp[ncl];
  int64_t p0 = 0, p1 = 0;
  if (t < ncl) {
    p0 = sp[t];
    p1 = sp[t + 1];
  }
  // S1, S2: a cell without terms keeps 0.0 for both
  double D = 0.0, C = 0.0;
  for (int64_t base = P0; base < P1; base += SUP_TILE) {
    const int m = (int)(P1 - base < SUP_TILE ? P1 - base : SUP_TILE);
#pragma unroll
    for (int k = 0; k < SUP_TILE / SUP_THREADS; k++) {
      const int q = k * SUP_THREADS + t;
      if (q < m) {
        const int64_t i = M.col[base + q];
        const double w = M.w[base + q], n = nleft[i];
        const double x = rate[i] * (didt * n);
        const double y = qirr[i] * didt;
        const bool checks = n == dnspd;  // S0
        tile_d[q] = w * (checks ? x : 0.0);
        tile_c[q] = w * ((!checks && n > 0.0 ? x : 0.0) + y);
      }
    }
    __syncthreads();
    const int64_t lo = p0 > base ? p0 : base, hi = p1 < base + m ? p1 : base + m;
    for (int64_t p = lo; p < hi; p++) {
      const double xd = tile_d[p - base], xc = tile_c[p - base];
      D = p == p0 ? xd : D + xd;
      C = p == p0 ? xc : C + xc;
    }
    __syncthreads();
  }
  if (t < ncl) {
    const int64_t c = c0 + t;
    const double ar = area[c];
    const double Vd = (D * 0.001) * ar, Vc = (C * 0.001) * ar;  // S3
    double a = volr[c] * (1.0 - thr);
    if constexpr (DAM) {
      if (dm.cap[c] > 0.0) {  // D7
        const double r = dm.res[c] - dm.smin[c];
        a = a + (r > 0.0 ? r : 0.0);
      }
    }
    if constexpr (CMD) {  // C6: every slot's loads are issued before the sum; an empty slot reads the cell's own rows and adds nothing
      int32_t d[CMD_NDEP];
      double cl[CMD_NDEP], rs[CMD_NDEP], sm[CMD_NDEP];
#pragma unroll
      for (int k = 0; k < CMD_NDEP; k++) d[k] = cm.dam[(int64_t)k * cld + c];
#pragma unroll
      for (int k = 0; k < CMD_NDEP; k++) {
        const int64_t j = d[k] >= 0 ? (int64_t)d[k] : c;
        cl[k] = cm.claim[(int64_t)k * cld + c];
        rs[k] = dm.res[j];
        sm[k] = dm.smin[j];
      }
#pragma unroll
      for (int k = 0; k < CMD_NDEP; k++) {
        const double r = rs[k] - sm[k];
        if (d[k] >= 0) a = a + cl[k] * (r > 0.0 ? r : 0.0);
      }
    }
    a = a - Vc;
    const double avail = a > 0.0 ? a : 0.0;
    const double ratio = Vd > avail ? avail / Vd : 1.0;  // S4
    ratio_s[t] = ratio;
    if (ratio != 1.0) limited = 1;  // (every writer stores the same word)
    // S6
    sup_st(sup + (int64_t)ELMK_IRRSUP_DEMAND * cld + c, Vd);
    sup_st(sup + (int64_t)ELMK_IRRSUP_COMMITTED * cld + c, Vc);
    sup_st(sup + (int64_t)ELMK_IRRSUP_RATIO * cld + c, ratio);
    const gptr<double> u = sup + (int64_t)ELMK_IRRSUP_UNMET_SUM * cld + c;
    sup_st(u, *u + (Vd - Vd * ratio));
  }
  __syncthreads();
  if (!limited) return;  // (uniform: read after the barrier)
  // S5
  for (int64_t q = P0 + t; q < P1; q += SUP_THREADS) {
    int lo = 0, hi = ncl;  // sp[lo] <= q < sp[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (sp[mid] <= q) lo = mid;
      else hi = mid;
    }
    const double r = ratio_s[lo];
    if (r != 1.0) {
      const int64_t i = M.col[q];
      if (nleft[i] == dnspd) sup_st(rate + i, rate[i] * r);
    }
  }
}

void launch_irrigation_supply(int64_t ncols, double* irr_rows, int64_t ld, int idt, const OGridMap& M, const double* area,
                              const double* volr, double thr, double* sup_rows, int64_t cld, hipStream_t st, const double* dam_rows,
                              const double* dam_tab, const int32_t* cmd_dam, const double* cmd_claim)
{
  if (ncols <= 0 || M.ncells <= 0) return;
  const int nspd = (14400 + (idt - 1)) / idt;
  const dim3 grid((unsigned)((M.ncells + SUP_CELLS - 1) / SUP_CELLS));
  if (dam_rows) {
    const SupDam<true> dm{(gptr<const double>)(dam_rows + DAM_RES * cld), (gptr<const double>)(dam_tab + DAM_SMIN * cld),
                          (gptr<const double>)(dam_tab + DAM_CAP * cld)};
    if (cmd_dam)
      hipLaunchKernelGGL((k_irrigation_supply<true, true>), grid, dim3(SUP_THREADS), 0, st, (gptr<double>)irr_rows, ld, idt, nspd, M,
                         (gptr<const double>)area, (gptr<const double>)volr, thr, (gptr<double>)sup_rows, cld, dm,
                         SupCmd<true>{(gptr<const int32_t>)cmd_dam, (gptr<const double>)cmd_claim});
    else
      hipLaunchKernelGGL((k_irrigation_supply<true, false>), grid, dim3(SUP_THREADS), 0, st, (gptr<double>)irr_rows, ld, idt, nspd, M,
                         (gptr<const double>)area, (gptr<const double>)volr, thr, (gptr<double>)sup_rows, cld, dm, SupCmd<false>{});
  } else {
    hipLaunchKernelGGL((k_irrigation_supply<false, false>), grid, dim3(SUP_THREADS), 0, st, (gptr<double>)irr_rows, ld, idt, nspd, M,
                       (gptr<const double>)area, (gptr<const double>)volr, thr, (gptr<double>)sup_rows, cld, SupDam<false>{}, SupCmd<false>{});
  }
}

}  // namespace elmk
