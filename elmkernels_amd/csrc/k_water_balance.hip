// k_water_balance.hip - the closed column water budget on the device (elmk_water_balance_*; include/elmk.h "water balance"): the water
// mass with the aquifer in it at the start and at the end of the step (BEGWB, ENDWB = ELM's TWS), total runoff QRUNOFF, the budget's
// error ERRH2O with the hydrology's runoff and drainage as its source/sink, and ELM's soil-water outputs TOTSOILLIQ, TOTSOILICE and
// SOILWATER_10CM.  k_conservation keeps the reference's hardwired hydrology_source_sink = 0.0 and stays what it is; this stage is the
// budget of a step that ran the soil hydrology.  elmkernels_amd/hydrology.py: water_balance_begin / water_balance_end restate W0 - W6 on
// the host, and this file follows them statement by statement.  No contraction (the Makefile's -ffp-contract=off), left-associative
// sums, `/` the correctly rounded fp64 division, plain IEEE comparisons; a NaN is stored as the canonical quiet NaN.
//
// One thread per column, 256-thread workgroups, every access a coalesced SoA row.  W1's forty level loads (twenty of h2osoi_ice, twenty
// of h2osoi_liq) are issued from a fully unrolled loop into registers before the running sum starts, so that they are all in flight
// together; the sum then runs in k_conservation's order.  W5 sums the ten active layers out of the same registers.  W6 loads the eleven
// interfaces and, for the one straddling layer, that layer's dz.  Bytes per column on the byte tally (fp64 state): 40 x 8 (ice, liq)
// + 3 x 8 (h2ocan, h2osno, h2osfc) + 11 x 8 (zisoi) + 8 (dz of the straddling layer) + 6 x 8 (forcing and flux fields) + 4 or 5 x 8
// (hydrology rows) + 8 (BEGWB) read, 6 x 8 written.
//
// The (min, max, sum) triples of ERRH2O, QRUNOFF and ENDWB come from k_cons_reduce1 / k_cons_reduce2 (k_surface_fluxes.hip:
// launch_min_max_sum), in elmk_evaluate_conservation's order.  The census of bad columns, !(fabs(ERRH2O) <= tol), is integer work: a
// wave butterfly and one atomic per wave, as k_flag_reduce.
//
// ELMK_WB_NT (0 = plain stores, the default; 1 = nontemporal stores of the rows) is the switch of the store A/B in
// tests/tools/water_balance_cost.py; DESIGN.md section 21 records what is known of it.
#include "elmk_dev.h"
#include "elmk_kernels.h"

#ifndef ELMK_WB_NT
#define ELMK_WB_NT 0
#endif

namespace elmk {

namespace {
constexpr int WN = ELMK_HYD_NLAYER;
static_assert(NLEVSNO + WN + 1 <= NLEVTOT + 1 && NLEVTOT == 20, "soil layer j is level 5 + j; twenty levels of ice and liq");
constexpr long long WB_NONE = 0x7fffffffffffffffll;

__device__ __forceinline__ void wb_st(gptr<double> p, double v)
{
  if (v != v) v = __builtin_nan("");
  if (ELMK_WB_NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}
__device__ __forceinline__ gptr<const double> wb_first(gptr<const double> p) { return p; }
__device__ __forceinline__ gptr<const double> wb_first(gptr<const double> p, gptr<const double>) { return p; }
__device__ __forceinline__ gptr<const double> wb_last(gptr<const double> p) { return p; }
__device__ __forceinline__ gptr<const double> wb_last(gptr<const double>, gptr<const double> p) { return p; }
}  // namespace

#define LV(f, lev) S->f[(int64_t)(lev) * ld + c]

// W0: BEGWB = dtbegin_column_h2o + WA
__global__ __launch_bounds__(256) void k_wb_begin(const DevState* __restrict__ S, gptr<const double> hyd, gptr<double> wb)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const double begwb = S->dtbegin_column_h2o[c];
  wb_st(wb + (int64_t)ELMK_WB_BEGWB * ld + c, begwb + hyd[(int64_t)ELMK_HYD_WA * ld + c]);
}

// W1 - W6.  FROST: QRUNOFF takes QFLX_DRAIN_PERCHED of the frost-table extension's rows hydf as well.  IRRIG: W4 takes the
// irrigation's QFLX_IRRIG row as a term of the input (ELM's BalanceCheck; include/elmk.h "irrigation").  The row is one more kernel
// argument, a pack that is empty without IRRIG, so that the two plain instantiations keep the kernel arguments, and with them every
// instruction, they had before the term existed.  LAND: W4 takes the floodplain infiltration's QFLX_H2OROF_DRAIN row as the last term of
// the input (include/elmk.h "floodplain infiltration", F4); its row is one more member of the pack, behind the irrigation's
template <bool FROST, bool IRRIG, bool LAND, class... Q>
__global__ __launch_bounds__(256) void k_water_balance(const DevState* __restrict__ S, gptr<const double> hyd, gptr<const double> hydf,
                                                       gptr<double> wb, double dt, Q... qirr)
{
  static_assert(sizeof...(Q) == (IRRIG ? 1 : 0) + (LAND ? 1 : 0), "the QFLX_IRRIG row exactly with IRRIG, the QFLX_H2OROF_DRAIN row with LAND");
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;

  // W1: the forty loads first, then the sum in k_conservation's order
  double ice[NLEVTOT], liq[NLEVTOT];
#pragma unroll
  for (int i = 0; i < NLEVTOT; ++i) {
    ice[i] = LV(h2osoi_ice, i);
    liq[i] = LV(h2osoi_liq, i);
  }
  double zi[WN + 1];
#pragma unroll
  for (int j = 0; j <= WN; j++) zi[j] = LV(zisoi, NLEVSNO + j);  // zi[0] = the surface, zi[j + 1] = the bottom of layer j
  const double h2osno = S->h2osno[c];
  double water = S->h2ocan[c] + h2osno + S->h2osfc[c];
#pragma unroll
  for (int i = 0; i < NLEVTOT; ++i) water = water + (ice[i] + liq[i]);

  // W2
  const double endwb = water + hyd[(int64_t)ELMK_HYD_WA * ld + c];

  // W3
  double q = hyd[(int64_t)ELMK_HYD_QFLX_SURF * ld + c] + hyd[(int64_t)ELMK_HYD_QFLX_H2OSFC_SURF * ld + c] +
             hyd[(int64_t)ELMK_HYD_QFLX_DRAIN * ld + c];
  if constexpr (FROST) q = q + hydf[(int64_t)ELMK_HYDF_QFLX_DRAIN_PERCHED * ld + c];
  const double qrunoff = q + S->qflx_snwcp_liq[c];

  // W4
  const double begwb = wb[(int64_t)ELMK_WB_BEGWB * ld + c];
  double errh2o;
  if constexpr (IRRIG && LAND)
    errh2o = endwb - begwb - ((((S->forc_rain[c] + S->forc_snow[c]) + wb_first(qirr...)[c]) + wb_last(qirr...)[c]) - qrunoff - S->qflx_evap_tot[c] - S->qflx_snwcp_ice[c]) * dt;
  else if constexpr (LAND)
    errh2o = endwb - begwb - (((S->forc_rain[c] + S->forc_snow[c]) + wb_last(qirr...)[c]) - qrunoff - S->qflx_evap_tot[c] - S->qflx_snwcp_ice[c]) * dt;
  else if constexpr (IRRIG)
    errh2o = endwb - begwb - (((S->forc_rain[c] + S->forc_snow[c]) + wb_first(qirr...)[c]) - qrunoff - S->qflx_evap_tot[c] - S->qflx_snwcp_ice[c]) * dt;
  else
    errh2o = endwb - begwb - (S->forc_rain[c] + S->forc_snow[c] - qrunoff - S->qflx_evap_tot[c] - S->qflx_snwcp_ice[c]) * dt;

  // W5: the ten active layers
  double totliq = 0.0, totice = 0.0;
#pragma unroll
  for (int j = 0; j < WN; j++) {
    totliq = totliq + liq[NLEVSNO + j];
    totice = totice + ice[NLEVSNO + j];
  }

  // W6: the water of the top 0.1 m
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < WN; j++) {
    if (zi[j + 1] <= 0.1) s = s + (liq[NLEVSNO + j] + ice[NLEVSNO + j]);
    else if (zi[j] < 0.1) s = s + (liq[NLEVSNO + j] + ice[NLEVSNO + j]) * ((0.1 - zi[j]) / LV(dz, NLEVSNO + j));
  }

  wb_st(wb + (int64_t)ELMK_WB_ERRH2O * ld + c, errh2o);
  wb_st(wb + (int64_t)ELMK_WB_QRUNOFF * ld + c, qrunoff);
  wb_st(wb + (int64_t)ELMK_WB_ENDWB * ld + c, endwb);
  wb_st(wb + (int64_t)ELMK_WB_SOILWATER_10CM * ld + c, s);
  wb_st(wb + (int64_t)ELMK_WB_TOTSOILLIQ * ld + c, totliq);
  wb_st(wb + (int64_t)ELMK_WB_TOTSOILICE * ld + c, totice);
}
#undef LV

// opens the census {nbad, first_bad_col} for k_wb_census; elmk_run (cursor not null): in ring row *cursor, to which the nine values of
// the three triples are copied from out as well
__global__ void k_wb_open(const double* __restrict__ out, double* __restrict__ ring, long long* __restrict__ census,
                          const int32_t* __restrict__ cursor)
{
  const int64_t row = cursor ? *cursor : 0;
  if (ring && threadIdx.x < 9) ring[row * 9 + threadIdx.x] = out[threadIdx.x];
  if (threadIdx.x == 0) {
    census[row * 2] = 0;
    census[row * 2 + 1] = WB_NONE;
  }
}

// W8: a column is bad iff !(fabs(err) <= tol); the count and the smallest bad index
__global__ __launch_bounds__(256) void k_wb_census(const double* __restrict__ err, int64_t n, double tol, long long* __restrict__ census,
                                                   const int32_t* __restrict__ cursor)
{
  const int64_t row = cursor ? *cursor : 0;
  unsigned long long cnt = 0;
  long long first = WB_NONE;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    if (!(fabs(err[c]) <= tol)) {
      cnt++;
      if (c < first) first = c;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_xor(cnt, off, 64);
    const long long o = __shfl_xor(first, off, 64);
    first = o < first ? o : first;
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd((unsigned long long*)(census + row * 2), cnt);
    atomicMin(census + row * 2 + 1, first);
  }
}

void launch_wb_begin(const DevState* S, int64_t n, const double* hyd_rows, double* wb_rows, hipStream_t st)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_wb_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, (gptr<const double>)hyd_rows, (gptr<double>)wb_rows);
}

void launch_water_balance(const DevState* S, int64_t n, int64_t ld, const double* hyd_rows, const double* frost_rows, double* wb_rows,
                          double dt, double tol, double* part, double* out, double* ring, long long* census, const int32_t* cursor,
                          hipStream_t st, const double* qirr, const double* qland)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const auto rows = [&](auto kernel, auto... q) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, S, (gptr<const double>)hyd_rows, (gptr<const double>)frost_rows, (gptr<double>)wb_rows,
                       dt, q...);
  };
  using P = gptr<const double>;
  const P q = (P)qirr, ql = (P)qland;
  if (qland && qirr) frost_rows ? rows(k_water_balance<true, true, true, P, P>, q, ql) : rows(k_water_balance<false, true, true, P, P>, q, ql);
  else if (qland) frost_rows ? rows(k_water_balance<true, false, true, P>, ql) : rows(k_water_balance<false, false, true, P>, ql);
  else if (qirr) frost_rows ? rows(k_water_balance<true, true, false, P>, q) : rows(k_water_balance<false, true, false, P>, q);
  else frost_rows ? rows(k_water_balance<true, false, false>) : rows(k_water_balance<false, false, false>);
  static_assert(ELMK_WB_QRUNOFF == ELMK_WB_ERRH2O + 1 && ELMK_WB_ENDWB == ELMK_WB_ERRH2O + 2, "the reduced rows are adjacent");
  const double* diag = wb_rows + (size_t)ELMK_WB_ERRH2O * (size_t)ld;
  launch_min_max_sum(diag, ld, n, 3, part, out, st);
  hipLaunchKernelGGL(k_wb_open, dim3(1), dim3(64), 0, st, out, ring, census, cursor);
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(k_wb_census, dim3((unsigned)blocks), dim3(256), 0, st, diag, n, tol, census, cursor);
}

}  // namespace elmk
