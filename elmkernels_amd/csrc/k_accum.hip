// k_accum.hip - accumulated fields on the device (elmk_accum_*; ELM's accumulMod): running means, period averages and running
// accumulations of state fields, updated once per step after the physics, with the result fed back into a state field (t10, the
// 10-day running mean of t_ref2m that photosynthesis' acclimation terms read) without a round trip through the host.
//
// The layout follows k_hist_accumulate: the unit of work is a row, one level of one entry (AccumRow, built on the host by
// elmk_accum_add); the grid is column-pair blocks x rows, so kind, stored dtype and period are uniform across a workgroup and every
// access is a coalesced SoA stream.  Every thread takes two adjacent columns (elmk_pair.h): a 16-byte load and store of the fp64
// value row, an 8-, 4- or 2-byte load of the source and a 16- or 8-byte store of the destination.  Bytes per column and row for an
// fp64 source with a destination: 8 + 16 + 8 = 32.
//
// Semantics (include/elmk.h, "accumulated fields"; elmkernels_amd/accum.py restates them in numpy), per element, with
// nstep = n + 1, n the updates folded into the entry so far, and v the stored sample widened to fp64; no contraction, `/` the
// correctly rounded fp64 division:
//   RUNMEAN   a = min(nstep, P);  val = ((double)(a - 1) * val + v) / (double)a
//   TIMEAVG   if (nstep % P == 1 || P == 1) val = +0.0;  val = val + v;  if (nstep % P == 0) val = val / (double)P
//   RUNACCUM  if (rint(v) == -99999.0) val = +0.0;  else t = val + v, t = t > 0.0 ? t : 0.0, val = t < 99999.0 ? t : 99999.0
// The destination receives val at state precision on every update (TIMEAVG: only on the update that completes a period).
//
// The step count lives on the device, so a captured update replayed N times advances it N times.  Every workgroup of
// k_accum_update reads its entry's count; the count is advanced by a one-thread kernel behind it (k_accum_next, as k_run_next
// advances the step cursor), which stream order places after every read.  The alternative, the last-workgroup-done counter of
// k_bg_flux, needs one atomic per workgroup on ONE address; at the ~14 ns per same-address atomic that DESIGN section 3 measured
// for k_bg_flux, the 19 532 workgroups per row at 10 M columns would queue for ~270 us (an estimate: the counter was not built).
// Measured (tests/tools/accum_cost.py, profiles/r13_accum_cost.jsonl): the t10 update, both launches, takes 0.0497 ms at 10 M
// columns (6.4 TB/s; 1.32 x elmk_history_accumulate with one single-level AVG entry, 4/3 expected from the bytes) and 0.0069 ms at
// 1 M (1.59 x: about 1 us over 4/3 of the history launch, which is what the second launch costs when the stream is that short).
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_pair.h"

namespace elmk {

namespace {
// the per-workgroup constants of one update of a row
struct AccumStep {
  int kind;
  double am1, a;   // RUNMEAN: (double)(a - 1), (double)a
  bool zero, div;  // TIMEAVG: first update of a period, last update of a period
  double p;        // TIMEAVG: (double)P
};

__device__ __forceinline__ double accum_fold(const AccumStep& s, double val, double v)
{
  switch (s.kind) {
    case ELMK_ACCUM_RUNMEAN: return (s.am1 * val + v) / s.a;
    case ELMK_ACCUM_TIMEAVG: {
      if (s.zero) val = 0.0;
      val = val + v;
      if (s.div) val = val / s.p;
      return val;
    }
    default: {  // ELMK_ACCUM_RUNACCUM
      if (__builtin_rint(v) == -99999.0) return 0.0;
      double t = val + v;
      t = t > 0.0 ? t : 0.0;
      return t < 99999.0 ? t : 99999.0;
    }
  }
}
}  // namespace

// grid (column pairs / 256, rows); rows[blockIdx.y] and its entry's count are uniform across the workgroup
__global__ __launch_bounds__(256) void k_accum_update(const AccumRow* __restrict__ rows, const unsigned long long* nsteps, int64_t npairs)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const AccumRow r = rows[blockIdx.y];
  const unsigned long long nstep = nsteps[r.entry] + 1ull, P = (unsigned long long)r.period;
  AccumStep s;
  s.kind = r.kind;
  const unsigned long long a = nstep < P ? nstep : P;
  s.am1 = (double)(a - 1ull);
  s.a = (double)a;
  s.zero = nstep % P == 1ull || P == 1ull;
  s.div = nstep % P == 0ull;
  s.p = (double)P;
  const hd2 v = load_pair(r.src, r.dtype, 2 * p);
  ELMK_GLOBAL hd2* q = (ELMK_GLOBAL hd2*)r.val + p;
  hd2 val = h_ld(q);
  val.x = accum_fold(s, val.x, v.x);
  val.y = accum_fold(s, val.y, v.y);
  h_st(q, val);
  if (!r.dst || (r.kind == ELMK_ACCUM_TIMEAVG && !s.div)) return;
  // The destination is stored plainly: interleaved A/B runs of tests/tools/accum_cost.py --ab (profiles/r13_accum_dst_nt_ab.jsonl)
  // against a build with the nontemporal hint on this store took the t10 update from 0.0070 to 0.0088 ms at 1 M columns and from
  // 0.0494 to 0.0518 ms at 10 M; inside elmk_run the two builds differ by less than the spread between two contexts.
  if (r.dst_f32) ((ELMK_GLOBAL hf2*)r.dst)[p] = hf2{(float)val.x, (float)val.y};
  else ((ELMK_GLOBAL hd2*)r.dst)[p] = val;
}

// after k_accum_update in stream order: every workgroup has read the counts
__global__ void k_accum_next(unsigned long long* nsteps, int nentries)
{
  for (int e = 0; e < nentries; e++) nsteps[e] += 1ull;
}

// grid (column pairs / 256, nlev): val = the stored source widened
__global__ __launch_bounds__(256) void k_accum_seed(const char* __restrict__ src, int dtype, int esize, double* __restrict__ val,
                                                    int64_t ld, int64_t npairs)
{
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const int64_t row = (int64_t)blockIdx.y * ld;
  ((ELMK_GLOBAL hd2*)(val + row))[p] = load_pair(src + row * esize, dtype, 2 * p);
}

static unsigned pair_blocks(int64_t npairs) { return (unsigned)(npairs > 0 ? (npairs + 255) / 256 : 1); }

void launch_accum_update(const AccumRow* rows, int nrows, unsigned long long* nsteps, int nentries, int64_t ncols, hipStream_t st)
{
  if (nrows <= 0) return;
  const int64_t npairs = (ncols + 1) / 2;
  hipLaunchKernelGGL(k_accum_update, dim3(pair_blocks(npairs), (unsigned)nrows), dim3(256), 0, st, rows, nsteps, npairs);
  hipLaunchKernelGGL(k_accum_next, dim3(1), dim3(1), 0, st, nsteps, nentries);
}

void launch_accum_seed(const void* src, int dtype, double* val, int nlev, int64_t ld, int64_t ncols, hipStream_t st)
{
  const int64_t npairs = (ncols + 1) / 2;
  const int esize = dtype == ELMK_F64 ? 8 : (dtype == ELMK_U8 ? 1 : 4);
  hipLaunchKernelGGL(k_accum_seed, dim3(pair_blocks(npairs), (unsigned)nlev), dim3(256), 0, st, (const char*)src, dtype, esize, val, ld,
                     npairs);
}

}  // namespace elmk
