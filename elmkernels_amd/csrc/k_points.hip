// k_points.hip - the point series (elmk_points_*; include/elmk.h "point series", P0 - P9): per-step records of chosen columns and river
// cells.  ONE launch per record gathers the current value of every (entry, point) pair into one slot of a device-resident ring
// [max_records][stride]; the same kernel serves the stepwise call and elmk_run's step.
//
// The unit of work is a wave.  A gather entry (a state field's level, a feature row, a cell row) of n points takes ceil(n / 64) waves, one
// thread per point: one load of the list, one dtype-aware load of the source, one store.  A gridded entry takes one wave per point: the wave
// walks the cell's span of the output grid's CSR map 64 terms at a time, every lane forming one product w[p] * x[col[p]] - one rounding
// whichever lane forms it - and the products are added in term order, v = x0, then v = v + x, the same chain in every lane; lane 0 stores
// the sum.  That is agg_cells' value (k_history.hip) and regrid.apply_aggregate's bit for bit, and a cell without terms reads fill.  A
// wave never straddles two entries (PointsEntry::wave0), so the entry's descriptor is wave-uniform: it is found by a search over at most
// 64 first-wave numbers and read from the device table through a readfirstlane'd index.
//
// The slot (P6): the stepwise call passes it; inside elmk_run's step - possibly a replayed graph, whose arguments are those of the
// capture - it is (*base + *cursor) % max_records, where cursor is the run's step cursor and base the word elmk_run writes on the stream
// before the run's first step, and the stamp is stamps[*cursor], the step's decday.  A record writes its slot and nothing else.
// Nothing is shared between threads: no read-modify-write, no fence, no hint on loads or stores - the data of a record is tiny and the
// launch is expected to cost its latency.
#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

namespace {
// one element of a source row widened to fp64 as the history's samples are (k_history.hip: load_one); fp64 is copied as stored
__device__ __forceinline__ double points_load(const void* src, int dtype, int64_t c)
{
  switch (dtype) {
    case ELMK_F64: return ((const ELMK_GLOBAL double*)src)[c];
    case ELMK_F32_STORED: return (double)((const ELMK_GLOBAL float*)src)[c];
    case ELMK_I32: return (double)((const ELMK_GLOBAL int32_t*)src)[c];
    case ELMK_U32: return (double)((const ELMK_GLOBAL uint32_t*)src)[c];
    default: return (double)((const ELMK_GLOBAL uint8_t*)src)[c];
  }
}
}  // namespace

// grid (ceil(nwaves / 4)) of 256 threads
__global__ __launch_bounds__(256) void k_points_record(const PointsTable* __restrict__ T, OGridMap M, double* __restrict__ ring, int64_t stride,
                                                       int max_records, int slot, double stamp, const int32_t* __restrict__ cursor,
                                                       const int32_t* __restrict__ base, const double* __restrict__ stamps)
{
  if (cursor) {  // (uniform: a kernel argument)
    const int32_t row = cursor[0];
    slot = (int)(((int64_t)base[0] + (int64_t)row) % (int64_t)max_records);
    stamp = stamps[row];
  }
  ELMK_GLOBAL double* rec = (ELMK_GLOBAL double*)ring + (int64_t)slot * stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = stamp;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (wave >= T->nwaves) return;
  int lo = 0, hi = T->nentries;  // e[lo].wave0 <= wave < e[hi].wave0 (e[nentries].wave0 would be nwaves)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (T->e[mid].wave0 <= wave) lo = mid;
    else hi = mid;
  }
  const PointsEntry e = T->e[lo];
  ELMK_GLOBAL double* out = rec + POINTS_HEAD + e.out;
  const ELMK_GLOBAL int64_t* list = (const ELMK_GLOBAL int64_t*)e.list;
  const int k = wave - e.wave0;
  if (!e.gridded) {
    const int i = k * 64 + lane;
    if (i < e.n) out[i] = points_load(e.src, e.dtype, list[i]);
    return;
  }
  // one wave, one cell: every lane walks the same span
  const int64_t cell = list[k];
  const int64_t p0 = M.ptr[cell], p1 = M.ptr[cell + 1];
  double v = M.fill;
  for (int64_t b = p0; b < p1; b += 64) {
    const int m = (int)(p1 - b < 64 ? p1 - b : 64);
    double prod = 0.0;
    if (lane < m) prod = M.w[b + lane] * points_load(e.src, e.dtype, M.col[b + lane]);
    for (int q = 0; q < m; q++) {
      const double x = __shfl(prod, q, 64);
      v = (b == p0 && q == 0) ? x : v + x;
    }
  }
  if (lane == 0) out[k] = v;
}

void launch_points_record(const PointsTable* T, int nwaves, const OGridMap& M, double* ring, int64_t stride, int max_records, int slot,
                          double stamp, const int32_t* cursor, const int32_t* base, const double* stamps, hipStream_t st)
{
  if (nwaves <= 0 || max_records <= 0) return;
  hipLaunchKernelGGL(k_points_record, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, st, T, M, ring, stride, max_records, slot, stamp, cursor,
                     base, stamps);
}

}  // namespace elmk
