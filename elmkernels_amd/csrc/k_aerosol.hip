// k_aerosol.hip - aerosol deposition from a monthly climatology (elmk_aerosol_*; ELM's aerdepini / aerinterp): the eleven deposition
// streams aer_bcphi .. aer_dst4_2 of aero_data::AerosolFileInput (src/data/aerosol_data.h:10-28), interpolated in time between two
// months of a resident series and in space through a map of the series' own grid.  The reference has the hook commented out at
// init_timestep_kokkos.cc:48-49 and never fills AerosolFileInput; aerosol_data_old_impl.hh:32-55 shows the two ingredients, the
// month bracket with its weights and a nearest-cell pick.  compute_aerosol_deposition (aerosol_physics_impl.hh:49-57, here in
// k_snow_hydrology.hip) reads the eleven fields every step and keeps the sums bcpho + bcdep, dstX_1 + dstX_2 and the * dtime.
//
// The series is cells[AER_NSTREAM][12][ncells] in fp64 (both builds).  Per stream s and column c, without contraction:
//   r1 = remap of cells[s][month1] to column c,  r2 = remap of cells[s][month2] to column c
//   aer_s[c] = wt1 * r1 + wt2 * r2          (two products and one sum, also when month1 == month2 or a weight is 0)
// The remap is elmk_set_forcing_grid's, in its operation order (k_forcing.hip: remap_cells; regrid.apply_map on the host), through a
// map of the aerosol grid's own: v = w[0] * a[idx[0]], then v = v + w[k] * a[idx[k]] for every k >= 1 with idx[k] >= 0.  NPTS = 0 is
// the per-column series (ncells == ncols): r = a[c], no map and no multiplication.  elmkernels_amd/aerosol.py: interpolate restates
// all of it in numpy.
//
// One thread per column.  The map row is loaded once (ELL rows are column-fastest: coalesced) and serves the 22 gathers; those hit a
// table of a few MB that stays in L2 / MALL, so nothing is staged in LDS.  NPTS is launch-uniform (1, 2, 4 or 8 with padding rows),
// so the term loop is unrolled per width.  Eleven coalesced stores per column at state precision (rounded to fp32 in
// libelmk_f32.so), with the store flavour the Makefile's FLAGS_k_aerosol gives this unit.  Bytes per column on the tally the cost
// tool uses: 88 written + NPTS x 12 of map read.  Every gather is inside a cell record: the host checked idx against ncells
// (elmk_aerosol_reserve) and the months against 0 .. 11 (elmk_aerosol_deposition, elmk_run) before anything was enqueued.
#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

namespace {
// one month of one stream as column c sees it (k_forcing.hip: load_map_row / remap_cells, restated here so that k_forcing.hip's
// kernels stay the text they were)
template <int NPTS> struct AerMapRow {
  int32_t idx[NPTS > 0 ? NPTS : 1];
  double w[NPTS > 0 ? NPTS : 1];
  __device__ __forceinline__ void load(gptr<const int32_t> midx, gptr<const double> mw, int64_t ld, int64_t c)
  {
#pragma unroll
    for (int k = 0; k < NPTS; k++) {
      idx[k] = midx[(int64_t)k * ld + c];
      w[k] = mw[(int64_t)k * ld + c];
    }
  }
  __device__ __forceinline__ double remap(gptr<const double> a, int64_t c) const
  {
    if constexpr (NPTS == 0) {
      return a[c];
    } else {
      double v = w[0] * a[idx[0]];
#pragma unroll
      for (int k = 1; k < NPTS; k++)
        if (idx[k] >= 0) v = v + w[k] * a[idx[k]];
      return v;
    }
  }
};

// one column: the body of both kernels
template <int NPTS>
__device__ __forceinline__ void aerosol_col(const DevState* __restrict__ S, int64_t c, gptr<const double> cells, int64_t ncells,
                                            gptr<const int32_t> midx, gptr<const double> mw, int64_t m1, int64_t m2, double wt1,
                                            double wt2)
{
  AerMapRow<NPTS> row;
  row.load(midx, mw, S->ld, c);
  const dfield dst[AER_NSTREAM] = {S->aer_bcphi,  S->aer_bcpho,  S->aer_bcdep,  S->aer_dst1_1, S->aer_dst1_2, S->aer_dst2_1,
                                   S->aer_dst2_2, S->aer_dst3_1, S->aer_dst3_2, S->aer_dst4_1, S->aer_dst4_2};
  // every gather before the first store: a store to a state field may alias the cell table as far as the compiler knows, so a loop
  // that stored each stream as it went waited for two gathers at a time, eleven L2 round trips in a row per column
  double v[AER_NSTREAM];
#pragma unroll
  for (int s = 0; s < AER_NSTREAM; s++) {
    const double r1 = row.remap(cells + ((int64_t)s * RUN_NMONTH + m1) * ncells, c);
    const double r2 = row.remap(cells + ((int64_t)s * RUN_NMONTH + m2) * ncells, c);
    v[s] = wt1 * r1 + wt2 * r2;
  }
#pragma unroll
  for (int s = 0; s < AER_NSTREAM; s++) dst[s][c] = v[s];
}
}  // namespace

// RUN: months and weights from the step's row of the device step table (elmk_run, as k_phenology_run reads them); otherwise the
// arguments (elmk_aerosol_deposition)
template <int NPTS, bool RUN>
__global__ __launch_bounds__(256) void k_aerosol_deposition(const DevState* __restrict__ S, gptr<const double> cells, int64_t ncells,
                                                            gptr<const int32_t> midx, gptr<const double> mw,
                                                            const RunRow* __restrict__ rows, const int32_t* __restrict__ cursor, int month1,
                                                            int month2, double wt1, double wt2)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S->ncols) return;
  if constexpr (RUN) {
    const RunRow* __restrict__ r = rows + *cursor;
    aerosol_col<NPTS>(S, c, cells, ncells, midx, mw, r->month1, r->month2, r->month_wt1, r->month_wt2);
  } else {
    aerosol_col<NPTS>(S, c, cells, ncells, midx, mw, month1, month2, wt1, wt2);
  }
}

template <bool RUN>
static void launch_aerosol(const DevState* S, int64_t n, const AerSeries& A, const RunRow* rows, const int32_t* cursor, int month1,
                           int month2, double wt1, double wt2, hipStream_t st)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const gptr<const double> a = (gptr<const double>)A.cells;
  const gptr<const int32_t> mi = (gptr<const int32_t>)A.idx;
  const gptr<const double> mw = (gptr<const double>)A.w;
#define ELMK_AER(N) hipLaunchKernelGGL((k_aerosol_deposition<N, RUN>), grid, block, 0, st, S, a, A.ncells, mi, mw, rows, cursor, month1, month2, wt1, wt2)
  switch (A.npad) {
    case 0: ELMK_AER(0); break;
    case 1: ELMK_AER(1); break;
    case 2: ELMK_AER(2); break;
    case 4: ELMK_AER(4); break;
    default: ELMK_AER(8); break;
  }
#undef ELMK_AER
}

void launch_aerosol_deposition(const DevState* S, int64_t n, const AerSeries& A, int month1, int month2, double wt1, double wt2,
                               hipStream_t st)
{
  launch_aerosol<false>(S, n, A, nullptr, nullptr, month1, month2, wt1, wt2, st);
}

void launch_aerosol_deposition_run(const DevState* S, int64_t n, const AerSeries& A, const RunRow* rows, const int32_t* cursor,
                                   hipStream_t st)
{
  launch_aerosol<true>(S, n, A, rows, cursor, 0, 0, 0.0, 0.0, st);
}

}  // namespace elmk
