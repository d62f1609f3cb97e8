// k_routing.hip - runoff routing on the device (elmk_routing_*; include/elmk.h "runoff routing"): the linear-reservoir river transport
// model of the CLM family (RTM) over the output grid's cells.  Every cell drains into one downstream cell; a call aggregates the water
// balance's QRUNOFF row onto the cells (R1) and takes nsub explicit sub-steps of the storages (R2 - R5).  elmkernels_amd/routing.py:
// call() restates the operation in numpy, and this file follows it statement by statement.  No contraction (the Makefile's
// -ffp-contract=off), plain IEEE comparisons, `/` the correctly rounded fp64 division; a NaN is stored into a row as the canonical
// quiet NaN.  Every row is fp64 in both builds, so both builds compile the same kernels.
//
// One thread per cell, 256-thread workgroups, no LDS, no atomics, no fences.  A sub-step reads the storages of its start from one
// buffer and writes the new ones into the other, so no cell sees a neighbour's update: the order between sub-steps is the launch
// boundary, and the two buffers are used in turn.  The chain starts in the buffer from which nsub sub-steps end in the VOLR row: for an
// odd nsub the R1 launch copies VOLR into the second buffer first.  The upstream map is stored [npad][ld], so a wave's index loads
// coalesce; the loop over its slots is unrolled over npad = ell_npad(largest in-degree), every slot's gather is issued whether the
// slot holds a cell or not (an empty slot reads the cell's own storage and adds nothing), so the loads of a cell are all in flight
// together.  The flow of an upstream cell is evaluated again from its storage rather than read from a row of flows: the same bits,
// one row less to write and read.  A cell reads 8 (storage) + 8 (KOUT) + 8 (QIN) + 4 npad (map) + 16 per upstream cell and, past the
// first sub-step, 8 (the flow sum), and writes 16.  The unit carries no nontemporal hint: none has been measured for it.
// The second scheme of the stage, kinematic-wave routing (k_kinematic_prep, k_kinematic_step), follows the linear one below, with its
// floodplain inundation (k_kinematic_step's FLOOD form), its reservoirs (both kernels' DAM form) and its stream temperature (the HEAT
// form: k_kinematic_prep<.., HEAT> and k_kinematic_step<.., HEAT>).
#include <type_traits>

#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

namespace {
__device__ __forceinline__ void route_st(gptr<double> p, double v)
{
  if (v != v) v = __builtin_nan("");
  *p = v;
}

// R2: what a storage v releases per second at rate constant k; the cap v / dts keeps a cell from releasing more than it holds
__device__ __forceinline__ double route_flow(double v, double k, double dts)
{
  if (!(v > 0.0)) return 0.0;
  const double a = v * k, b = v / dts;
  return a < b ? a : b;
}
}  // namespace

// R1: QIN of every cell from the column rows through the output grid's CSR map, in the order of k_ogrid_aggregate's sums; a cell
// without terms takes +0.0.  WITHDRAW: the irrigation's QFLX_IRRIG row is aggregated the same way and subtracted.  volr_b not null: the
// storages are copied into the second buffer (an odd nsub starts there).
template <bool WITHDRAW>
__global__ __launch_bounds__(256) void k_routing_qin(gptr<const int64_t> ptr, gptr<const int32_t> col, gptr<const double> w,
                                                     gptr<const double> qrunoff, gptr<const double> qirr, gptr<const double> area,
                                                     gptr<double> qin, gptr<const double> volr, gptr<double> volr_b, int64_t ncells)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  const int64_t p0 = ptr[c], p1 = ptr[c + 1];
  double r = 0.0, i = 0.0;
  for (int64_t p = p0; p < p1; p++) {
    const int32_t k = col[p];
    const double wp = w[p];
    const double x = wp * qrunoff[k];
    r = p == p0 ? x : r + x;
    if constexpr (WITHDRAW) {
      const double y = wp * qirr[k];
      i = p == p0 ? y : i + y;
    }
  }
  if constexpr (WITHDRAW) r = r - i;
  route_st(qin + c, (r * 0.001) * area[c]);
  if (volr_b) volr_b[c] = volr[c];
}

// R3 - R5: one sub-step.  FIRST: the flow sum starts at +0.0; otherwise it continues from the QOUT row.  LAST: QOUT takes the mean
// over the sub-steps and QOUT_SUM adds it.
template <int NPAD, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_routing_step(gptr<const double> v_old, gptr<double> v_new, gptr<const double> kout,
                                                      gptr<const int32_t> up, gptr<const double> qin, gptr<double> qout,
                                                      gptr<double> qout_sum, int64_t ncells, int64_t cld, double dts, double dnsub)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  int32_t u[NPAD];
#pragma unroll
  for (int p = 0; p < NPAD; p++) u[p] = up[(int64_t)p * cld + c];
  const double v = v_old[c], k = kout[c], q = qin[c];
  double qacc = 0.0;
  if constexpr (!FIRST) qacc = qout[c];
  double vu[NPAD], ku[NPAD];
#pragma unroll
  for (int p = 0; p < NPAD; p++) {
    const int64_t j = u[p] >= 0 ? (int64_t)u[p] : c;
    vu[p] = v_old[j];
    ku[p] = kout[j];
  }
  const double f = route_flow(v, k, dts);
  double fin = 0.0;
#pragma unroll
  for (int p = 0; p < NPAD; p++) {
    const double fu = route_flow(vu[p], ku[p], dts);
    if (u[p] >= 0) fin = fin + fu;
  }
  route_st(v_new + c, v + ((fin - f) + q) * dts);
  qacc = qacc + f;
  if constexpr (LAST) {
    const double mean = qacc / dnsub;
    route_st(qout + c, mean);
    route_st(qout_sum + c, qout_sum[c] + mean);
  } else {
    route_st(qout + c, qacc);
  }
}

// R6's third row: QOUT of the outlets, +0.0 elsewhere
__global__ __launch_bounds__(256) void k_routing_outlets(gptr<const int32_t> down, gptr<const double> qout, gptr<double> outlet,
                                                         int64_t ncells)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  outlet[c] = down[c] < 0 ? qout[c] : 0.0;
}

namespace {
// A run-time value as a compile-time one: f is called with the std::integral_constant of the value, and the kernel's template
// arguments are read off the constants' types where the launch is spelled out.
template <class F>
void with_bool(bool b, F f)
{
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// npad = ell_npad(largest in-degree): 1, 2, 4 or 8
template <class F>
void with_npad(int npad, F f)
{
  switch (npad) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}
}  // namespace

void launch_routing(const RouteArgs& A, const OGridMap& M, const double* qrunoff, const double* qirr, double dt, hipStream_t st)
{
  if (A.ncells <= 0) return;
  const dim3 grid((unsigned)((A.ncells + 255) / 256)), block(256);
  double* const volr = A.rows + ROUTE_VOLR * A.cld;
  double* const volr_b = A.rows + ROUTE_VOLR_B * A.cld;
  const bool odd = (A.nsub & 1) != 0;
  const auto qin = qirr ? k_routing_qin<true> : k_routing_qin<false>;
  hipLaunchKernelGGL(qin, grid, block, 0, st, (gptr<const int64_t>)M.ptr, (gptr<const int32_t>)M.col, (gptr<const double>)M.w,
                     (gptr<const double>)qrunoff, (gptr<const double>)qirr, (gptr<const double>)A.area,
                     (gptr<double>)(A.rows + ROUTE_QIN * A.cld), (gptr<const double>)volr, (gptr<double>)(odd ? volr_b : nullptr), A.ncells);
  const double dts = dt / (double)A.nsub;  // R0
  double *src = odd ? volr_b : volr, *dst = odd ? volr : volr_b;
  for (int s = 0; s < A.nsub; s++) {
    with_npad(A.npad, [&](auto npad) {
      with_bool(s == 0, [&](auto first) {
        with_bool(s == A.nsub - 1, [&](auto last) {
          hipLaunchKernelGGL((k_routing_step<decltype(npad)::value, decltype(first)::value, decltype(last)::value>), grid, block, 0, st,
                             (gptr<const double>)src, (gptr<double>)dst, (gptr<const double>)A.kout, (gptr<const int32_t>)A.up,
                             (gptr<const double>)(A.rows + ROUTE_QIN * A.cld), (gptr<double>)(A.rows + ROUTE_QOUT * A.cld),
                             (gptr<double>)(A.rows + ROUTE_QOUT_SUM * A.cld), A.ncells, A.cld, dts, (double)A.nsub);
        });
      });
    });
    double* const t = src;
    src = dst;
    dst = t;
  }
}

void launch_routing_outlets(const RouteArgs& A, const int32_t* down, hipStream_t st)
{
  if (A.ncells <= 0) return;
  hipLaunchKernelGGL(k_routing_outlets, dim3((unsigned)((A.ncells + 255) / 256)), dim3(256), 0, st, (gptr<const int32_t>)down,
                     (gptr<const double>)(A.rows + ROUTE_QOUT * A.cld), (gptr<double>)(A.rows + ROUTE_OUTLET * A.cld), A.ncells);
}

// ---- kinematic-wave routing (include/elmk.h "kinematic-wave routing", K0 - K9; elmkernels_amd/routing.py: kinematic_call) ----------
// The second scheme of the stage: three stores per cell (hillslope WH, tributaries WT, main channel VOLR), each released by Manning's
// equation.  One thread per cell and 256-thread workgroups as above.  A cell's own three storages are read and written by its own
// thread only, so they update in place; what crosses cells is the main channel's flow er, and it goes through a row of flows in two
// buffers: the K1 launch writes the er of the call's first sub-step, every sub-step but the last writes the er of its new VOLR into
// the other buffer, and the next sub-step gathers from there.  That is the same operands through the same operations as evaluating
// er again from the upstream storages (the linear kernel's way), at 8 bytes per upstream slot instead of a pow, four divisions and four
// gathers.  pow is elmk_pow with its tables in global memory: a thread evaluates it three times per launch, outside any loop, and a
// workgroup's copy of the tables into LDS (elmk_math_lds_init: 7 KB, 3.5 loads per thread) would cost as many vector-memory loads as
// the lookups it saves; the 5 KB the three evaluations touch stay in L1 / L2.  No LDS, no fences, no nontemporal hint (no A/B run).
namespace {
constexpr double KW_T23 = 2.0 / 3.0, KW_T53 = 5.0 / 3.0;

// K2 with the rate formed only where it is taken (K9: any other storage releases nothing)
// K3
__device__ __forceinline__ double kw_hill(double wh, double area, double ch, double dts)
{
  if (!(area > 0.0) || !(wh > 0.0)) return 0.0;
  const double h = wh / area;
  const double a = (ch * elmk_pow(h, KW_T53)) * area, b = wh / dts;
  return a < b ? a : b;
}
// K4
__device__ __forceinline__ double kw_chan(double w, double len, double wid, double c, double dts)
{
  if (!(w > 0.0)) return 0.0;
  const double a = w / len;
  const double y = a / wid;
  const double p = wid + 2.0 * y;
  const double r = a / p;
  const double q = (c * elmk_pow(r, KW_T23)) * a, b = w / dts;
  return q < b ? q : b;
}
}  // namespace

// ---- reservoirs (include/elmk.h "reservoirs", D0 - D8; elmkernels_amd/routing.py: reservoir_prep, reservoir_regulate) ---------------
// The DAM form of both kernels: a dam stands at the outlet of a cell with CAP > 0.0 and regulates the main channel's er where K4 forms
// it.  Every cell of the form reads CAP, 8 bytes; a dam cell reads SMIN, BETA, TARGET[m], KRLS and RES and writes RES and its natural
// er (the row DAM_ENAT, which its own thread reads back in the coming sub-step: D4), 56 bytes, all behind the cell's own condition.
// The month and `begins` are uniform over the launch: an argument, or the bits of the run row's pad word.
// D4's other choice, evaluating K4 again from the VOLR of the sub-step's start instead of keeping the row, is -DELMK_DAM_REEVAL (make
// variant V=damreeval VFLAGS=-DELMK_DAM_REEVAL): the same bits, measured by tests/tools/cost_routing_reservoir.py.
template <bool DAM>
struct DamRows {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct DamRows<true> {
  gptr<double> rows;           // [DAM_NROWS][cld]
  gptr<const double> tab;      // [DAM_NTAB][cld]
  gptr<const int32_t> mstart;  // [cld]
  const RunRow* run;
  const int32_t* cursor;
  int32_t time;
  double dt;
};

namespace {
__device__ __forceinline__ int32_t dam_time(const DamRows<true>& dm)
{
  const int32_t t = dm.run ? dm.run[*dm.cursor].pad >> RUN_PAD_DAM_SHIFT : dm.time;
  const int32_t m = t & 15;
  return (m > 11 ? 11 : m) | (t & 16);  // (the host hands 0 .. 11: TARGET's row stays inside the table whatever the word holds)
}
// D3 for a dam cell; e: the natural er.  Stores RES and DAM_ENAT, returns the regulated flow (a NaN as the canonical one)
__device__ __forceinline__ double dam_regulate(double e, double res, double krls, double cap, int32_t m, const DamRows<true>& dm,
                                               int64_t cld, int64_t c, double dts)
{
  const double smin = dm.tab[DAM_SMIN * cld + c], beta = dm.tab[DAM_BETA * cld + c], tgt = dm.tab[(DAM_TARGET + m) * cld + c];
  double q = beta * (krls * tgt) + (1.0 - beta) * e;
  const double qmin = 0.1 * e;
  if (q < qmin) q = qmin;
  double eo;
  if (q > e) {
    const double a = res - smin;
    double x = q - e;
    const double lim = a > 0.0 ? a / dts : 0.0;
    if (x > lim) x = lim;
    eo = e + x;
  } else {
    eo = q;
  }
  double s = res + (e - eo) * dts;
  if (s > cap) {
    eo = eo + (s - cap) / dts;
    s = cap;
  }
  route_st(dm.rows + (DAM_RES * cld + c), s);
#ifndef ELMK_DAM_REEVAL
  dm.rows[DAM_ENAT * cld + c] = e;
#endif
  if (eo != eo) eo = __builtin_nan("");
  return eo;
}
}  // namespace

// ---- stream temperature (include/elmk.h "stream temperature", H0 - H9; elmkernels_amd/routing.py: heat_prep, heat_phi, heat_settle) ----
// The HEAT form of both kernels: the tributary store and the main channel carry a temperature.  The K1 launch walks the map once for
// the water's three sums and H1's eight aggregates - sixteen more registers, still one wave's worth of loads per term in flight - and
// leaves what the sub-steps need of them as eight rows, so a sub-step reads rows and never the map.  What crosses cells is the heat
// flow hr = er * TR, in two buffers used in turn with er's.  AT, ACHN, WMINT and WMINR are formed from the scheme's parameter rows with
// H0's operations: the host's bits at 0 bytes instead of four rows.  A sub-step of the form reads TT, TR, hr, H1's eight rows and the
// four running diagnostics, 120 bytes and 8 per upstream slot, and writes TT, TR, the four diagnostics and hr (or HEAT), 56 bytes.
// Two exp and four divisions per cell at most, each behind the cell's own condition; no atomics, no LDS, no scratch.
template <bool HEAT>
struct HeatRows {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct HeatRows<true> {
  gptr<double> rows;         // [HT_NROWS][cld]
  gptr<const double> ksw;    // [cld] (the K1 launch)
  const void* f[HTF_N];      // the state fields of H1, as stored (the K1 launch)
  int dtype;                 // ELMK_F64 or ELMK_F32_STORED
  int64_t ld, tsub_off;      // the fields' level stride; the element offset of level 5 + sublev
  double ems0;               // H0
  gptr<const double> hr_old;  // the heat flows of the sub-step's start (the K1 launch: not read)
  gptr<double> hr_new;        // those of its end (the K1 launch: the first sub-step's)
};

namespace {
constexpr double HT_TFRZ = 273.15, HT_TMAX = 313.15, HT_RHOCP = 4188000.0, HT_EMIS = 0.97, HT_CPAIR = 1004.64, HT_LV = 2.501e6,
                 HT_RAIR = 287.04, HT_CEX = 1.3e-3, HT_DMIN = 1e-3;

// a state field's element as stored, widened
__device__ __forceinline__ double heat_ld(const void* p, int dtype, int64_t i)
{
  return dtype == ELMK_F32_STORED ? (double)((const ELMK_GLOBAL float*)p)[i] : ((const ELMK_GLOBAL double*)p)[i];
}
__device__ __forceinline__ double heat_fl(double t) { return t > HT_TFRZ ? t : HT_TFRZ; }

struct HeatCell {
  double rad, ke, ems, ta, qa, pa;
};
// H2
__device__ __forceinline__ double heat_phi(double T, const HeatCell& x)
{
  const double d = T - HT_TFRZ;
  const double es = 611.2 * elmk_exp((17.67 * d) / (T - 29.65));
  const double qs = (0.622 * es) / (x.pa - 0.378 * es);
  const double t2 = T * T;
  return (x.rad - x.ems * (t2 * t2)) + (x.ke * (HT_CPAIR * (x.ta - T) - HT_LV * (qs - x.qa))) / HT_RHOCP;
}
// H5
__device__ __forceinline__ double heat_settle(double h, double wn, double wmin, double teq, double& adj)
{
  double t = teq;
  bool acted = true;
  if (wn > wmin) {
    t = h / wn;
    acted = false;
    if (!(t >= HT_TFRZ)) t = HT_TFRZ, acted = true;
    if (t > HT_TMAX) t = HT_TMAX, acted = true;
  }
  adj = acted ? t * wn - h : 0.0;
  return t;
}
}  // namespace

// ---- floodplain infiltration (include/elmk.h "floodplain infiltration", F5; elmkernels_amd/routing.py: kinematic_call's land) ----------
// The LAND form of the K1 launch: one more sum in the CSR walk, 8 bytes per term; per cell WF read and written and QLAND written, 24 bytes.
template <bool LAND>
struct LandRows {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct LandRows<true> {
  gptr<const double> qdrain;  // [ld]: the column row QFLX_H2OROF_DRAIN
  gptr<double> wf, qland;     // [cld]
  double dt;
};

// ---- command areas (include/elmk.h "command areas", C0 - C8; elmkernels_amd/routing.py: command_allot, command_take) -------------------
// The CMD form of the K1 launch (k_kinematic_prep_cmd): a cell with a filled slot (dam[0] >= 0: slots fill from slot 0) reads 4 bytes more and writes WANT.
template <bool CMD>
struct CmdRows {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct CmdRows<true> {
  gptr<const int32_t> dam0;  // [cld]: slot 0 of the cells' ELL row
  gptr<double> want;         // [cld]
};

// K1: QIN as k_routing_qin, QSUR from the hydrology's two surface rows in the same order, QSUB, and the er of the first sub-step.
// DAM: D1, D2 and the first sub-step's D3 for the dam cells.  HEAT: H1.  LAND: F5.  CMD: C1.  The body of both kernels below.
namespace {
template <bool WITHDRAW, bool DAM, bool HEAT, bool LAND, bool CMD>
__device__ __forceinline__ void kinematic_prep(gptr<const int64_t> ptr, gptr<const int32_t> col, gptr<const double> w,
                                               gptr<const double> qrunoff, gptr<const double> qirr, gptr<const double> qsurf,
                                               gptr<const double> qh2osfc, gptr<const double> area, gptr<const double> volr,
                                               gptr<const double> par, gptr<double> qin, gptr<double> qsur, gptr<double> qsub,
                                               gptr<double> er, int64_t ncells, int64_t cld, double dts, DamRows<DAM> dm,
                                               HeatRows<HEAT> ht, LandRows<LAND> ln, CmdRows<CMD> cm)
{
  static_assert(!(HEAT && DAM), "the heat and the reservoirs exclude each other");
  static_assert(!(HEAT && LAND), "the heat excludes the inundation, and the infiltration with it");
  static_assert(!CMD || (WITHDRAW && DAM), "the command areas need the withdrawal and the reservoirs");
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  const int64_t p0 = ptr[c], p1 = ptr[c + 1];
  double r = 0.0, i = 0.0, s = 0.0;
  [[maybe_unused]] double tl = 0.0;
  [[maybe_unused]] double ta = 0.0, pa = 0.0, qa = 0.0, lw = 0.0, ua = 0.0, sw = 0.0, tsur = 0.0, tsub = 0.0;
  for (int64_t p = p0; p < p1; p++) {
    const int32_t k = col[p];
    const double wp = w[p];
    const double x = wp * qrunoff[k];
    r = p == p0 ? x : r + x;
    if constexpr (WITHDRAW) {
      const double y = wp * qirr[k];
      i = p == p0 ? y : i + y;
    }
    const double z = wp * (qsurf[k] + qh2osfc[k]);
    s = p == p0 ? z : s + z;
    if constexpr (LAND) {
      const double y = wp * ln.qdrain[k];
      tl = p == p0 ? y : tl + y;
    }
    if constexpr (HEAT) {  // H1's terms
      const bool first = p == p0;
      const int dt_ = ht.dtype;
      const double fu = heat_ld(ht.f[HTF_U], dt_, k), fv = heat_ld(ht.f[HTF_V], dt_, k);
      const double xt = wp * heat_ld(ht.f[HTF_TBOT], dt_, k), xp = wp * heat_ld(ht.f[HTF_PBOT], dt_, k);
      const double xq = wp * heat_ld(ht.f[HTF_QBOT], dt_, k), xl = wp * heat_ld(ht.f[HTF_LWRAD], dt_, k);
      const double xu = wp * sqrt(fu * fu + fv * fv);
      const double xs = wp * (((heat_ld(ht.f[HTF_SOLAD], dt_, k) + heat_ld(ht.f[HTF_SOLAD], dt_, ht.ld + k)) +
                               heat_ld(ht.f[HTF_SOLAI], dt_, k)) + heat_ld(ht.f[HTF_SOLAI], dt_, ht.ld + k));
      const double xg = wp * heat_fl(heat_ld(ht.f[HTF_TGRND], dt_, k));
      const double xb = wp * heat_fl(heat_ld(ht.f[HTF_TSOISNO], dt_, ht.tsub_off + k));
      ta = first ? xt : ta + xt;
      pa = first ? xp : pa + xp;
      qa = first ? xq : qa + xq;
      lw = first ? xl : lw + xl;
      ua = first ? xu : ua + xu;
      sw = first ? xs : sw + xs;
      tsur = first ? xg : tsur + xg;
      tsub = first ? xb : tsub + xb;
    }
  }
  [[maybe_unused]] const double rn = r;
  if constexpr (WITHDRAW) r = r - i;
  const double ar = area[c];
  const double q = (r * 0.001) * ar, qs = (s * 0.001) * ar;
  if constexpr (LAND) {  // F5
    const double ql = (tl * 0.001) * ar;
    route_st(ln.qland + c, ql);
    route_st(ln.wf + c, ln.wf[c] - ql * ln.dt);
  }
  if constexpr (DAM) {
    const double cap = dm.tab[DAM_CAP * cld + c];
    if (cap > 0.0) {  // D0
      const int32_t t = dam_time(dm), m = t & 15;
      double res = dm.rows[DAM_RES * cld + c], krls = dm.rows[DAM_KRLS * cld + c];
      if ((t & 16) && m == dm.mstart[c]) {  // D1
        krls = res / dm.tab[DAM_C85 * cld + c];
        route_st(dm.rows + (DAM_KRLS * cld + c), krls);
      }
      double take = 0.0, qd = q;
      if constexpr (WITHDRAW) {  // D2
        const double iv = (i * 0.001) * ar;
        const double want = iv * dm.dt;
        const double a = res - dm.tab[DAM_SMIN * cld + c];
        const double avail = a > 0.0 ? a : 0.0;
        take = want > avail ? avail : want;
        res = res - take;
        qd = (rn * 0.001) * ar - (iv - take / dm.dt);
        if constexpr (CMD) {  // C1: what the own dam did not cover
          if (cm.dam0[c] >= 0) {
            const double rest = iv - take / dm.dt;
            cm.want[c] = rest > 0.0 ? rest * dm.dt : 0.0;
          }
        }
      }
      route_st(dm.rows + (DAM_TAKE * cld + c), take);
      route_st(qin + c, qd);
      route_st(qsur + c, qs);
      route_st(qsub + c, qd - qs);
      const double e = kw_chan(volr[c], par[KW_RLEN * cld + c], par[KW_RWIDTH * cld + c], par[KW_CR * cld + c], dts);
      er[c] = dam_regulate(e, res, krls, cap, m, dm, cld, c, dts);  // D3
      return;
    }
  }
  route_st(qin + c, q);
  route_st(qsur + c, qs);
  route_st(qsub + c, q - qs);
  if constexpr (CMD) {  // C1
    if (cm.dam0[c] >= 0) {
      const double rest = (i * 0.001) * ar;
      cm.want[c] = rest > 0.0 ? rest * dm.dt : 0.0;
    }
  }
  const double e0 = kw_chan(volr[c], par[KW_RLEN * cld + c], par[KW_RWIDTH * cld + c], par[KW_CR * cld + c], dts);
  er[c] = e0;
  if constexpr (HEAT) {  // H1
    double rad = 0.0, ke = 0.0, ems = 0.0;
    if (p1 > p0) {
      rad = (ht.ksw[c] * sw + HT_EMIS * lw) / HT_RHOCP;
      ke = ((pa / (HT_RAIR * ta)) * HT_CEX) * ua;
      ems = ht.ems0;
    } else {
      tsur = tsub = HT_TFRZ;
      ta = qa = pa = 0.0;
    }
    route_st(ht.rows + (HT_RAD * cld + c), rad);
    route_st(ht.rows + (HT_KE * cld + c), ke);
    route_st(ht.rows + (HT_EMS * cld + c), ems);
    route_st(ht.rows + (HT_TA * cld + c), ta);
    route_st(ht.rows + (HT_QA * cld + c), qa);
    route_st(ht.rows + (HT_PA * cld + c), pa);
    route_st(ht.rows + (HT_TSUR * cld + c), tsur);
    route_st(ht.rows + (HT_TSUB * cld + c), tsub);
    ht.rows[HT_HEAT * cld + c] = 0.0;
    ht.rows[HT_HIN * cld + c] = 0.0;
    ht.rows[HT_HSRF * cld + c] = 0.0;
    ht.rows[HT_HADJ * cld + c] = 0.0;
    ht.rows[HT_HOUT * cld + c] = 0.0;
    route_st(ht.hr_new + c, e0 * ht.rows[HT_TR * cld + c]);
  }
}
}  // namespace

template <bool WITHDRAW, bool DAM = false, bool HEAT = false, bool LAND = false>
__global__ __launch_bounds__(256) void k_kinematic_prep(gptr<const int64_t> ptr, gptr<const int32_t> col, gptr<const double> w,
                                                        gptr<const double> qrunoff, gptr<const double> qirr, gptr<const double> qsurf,
                                                        gptr<const double> qh2osfc, gptr<const double> area, gptr<const double> volr,
                                                        gptr<const double> par, gptr<double> qin, gptr<double> qsur, gptr<double> qsub,
                                                        gptr<double> er, int64_t ncells, int64_t cld, double dts, DamRows<DAM> dm,
                                                        HeatRows<HEAT> ht, LandRows<LAND> ln)
{
  kinematic_prep<WITHDRAW, DAM, HEAT, LAND, false>(ptr, col, w, qrunoff, qirr, qsurf, qh2osfc, area, volr, par, qin, qsur, qsub, er, ncells, cld,
                                                   dts, dm, ht, ln, CmdRows<false>{});
}
// the CMD form of the K1 launch (C1): the withdrawal and the reservoirs are on
template <bool LAND>
__global__ __launch_bounds__(256) void k_kinematic_prep_cmd(gptr<const int64_t> ptr, gptr<const int32_t> col, gptr<const double> w,
                                                            gptr<const double> qrunoff, gptr<const double> qirr, gptr<const double> qsurf,
                                                            gptr<const double> qh2osfc, gptr<const double> area, gptr<const double> volr,
                                                            gptr<const double> par, gptr<double> qin, gptr<double> qsur, gptr<double> qsub,
                                                            gptr<double> er, int64_t ncells, int64_t cld, double dts, DamRows<true> dm,
                                                            LandRows<LAND> ln, CmdRows<true> cm)
{
  kinematic_prep<true, true, false, LAND, true>(ptr, col, w, qrunoff, qirr, qsurf, qh2osfc, area, volr, par, qin, qsur, qsub, er, ncells, cld, dts,
                                                dm, HeatRows<false>{}, ln, cm);
}

// ---- floodplain inundation (include/elmk.h "floodplain inundation", I0 - I8; elmkernels_amd/routing.py: inundation_exchange) --------
// The flood form of the sub-step: between K6's new VOLR and its store, the cell's channel and floodplain are brought to one water
// level.  A cell whose river is inside its banks and whose floodplain is dry (I1) reads VC and WF, 16 bytes, and nothing else of the
// tables; the 22 rows of the profile (E_0 .. E_10, VB_1 .. VB_10, ACHN, AF: 184 bytes) are loaded behind the cell's own condition, all
// at once so that they are in flight together, and the segment is found by a compare-and-select chain over them: the arrays are
// indexed by unrolled constants only, so they live in registers and the kernel has no scratch.  S_k, DE_k and M_k are formed again from
// ACHN, AF and the E_k with I0's operations, which gives the host's bits at 0 bytes instead of 31 more rows.  The two diagnostics are
// stored by the LAST sub-step only: every sub-step would overwrite them, and nothing reads them in between.
template <bool FLOOD>
struct FloodRows {};  // the plain form takes nothing: its kernel arguments, instructions and registers stay what they were
template <>
struct FloodRows<true> {
  gptr<double> rows;       // [FP_NROWS][cld]
  gptr<const double> tab;  // [FP_NTAB][cld]
};

namespace {
// I2 - I4 for a cell that I1 lets in; v: K6's VOLR on entry, the channel's share on return; wf likewise.  h, f: the diagnostics.
__device__ __forceinline__ void fp_exchange(double& v, double& wf, double& h, double& f, double vc, double ar, gptr<const double> tab,
                                            int64_t cld, int64_t c)
{
  const double W = v + wf;
  if (!(W > vc)) {  // I2 (a NaN comes here)
    v = W;
    wf = 0.0;
    return;
  }
  const double achn = tab[FP_ACHN * cld + c], af = tab[FP_AF * cld + c];
  double E[11], VB[11];
#pragma unroll
  for (int k = 0; k < 11; k++) E[k] = tab[(FP_E + k) * cld + c];
  VB[0] = 0.0;
#pragma unroll
  for (int k = 1; k < 11; k++) VB[k] = tab[(FP_VB + k) * cld + c];
  const double X = W - vc;  // I3
  double frac;
  if (X >= VB[10]) {
    const double s10 = achn + af * (10.0 / 10.0);
    h = E[10] + (X - VB[10]) / s10;
    frac = 1.0;
  } else {
    double vbk = VB[0], ek = E[0], ek1 = E[1], fk = 0.0 / 10.0;
#pragma unroll
    for (int k = 1; k < 10; k++) {
      const bool in = X >= VB[k];
      vbk = in ? VB[k] : vbk;
      ek = in ? E[k] : ek;
      ek1 = in ? E[k + 1] : ek1;
      fk = in ? (double)k / 10.0 : fk;
    }
    const double sk = achn + af * fk, de = ek1 - ek;
    const double mk = (af * 0.1) / de;
    const double r = X - vbk;
    double d = (2.0 * r) / (sk + sqrt(sk * sk + (2.0 * mk) * r));
    if (d > de) d = de;
    h = ek + d;
    frac = fk + (0.1 * d) / de;
  }
  double vc2 = vc + achn * h;  // I4
  if (vc2 > W) vc2 = W;
  v = vc2;
  wf = W - vc2;
  f = ar > 0.0 ? (af * frac) / ar : 0.0;
}
}  // namespace

// K3 - K7: one sub-step.  er_old: the flows of the sub-step's start; er_new: those of its end (not written by the LAST one).  FIRST and
// LAST as k_routing_step's.  FLOOD: the flood form, I1 - I5.  DAM: a dam cell's K6 subtracts its natural er (D4), and the er it forms
// is regulated (D3).  HEAT: H3 - H6 beside the water.
template <int NPAD, bool FIRST, bool LAST, bool FLOOD, bool DAM = false, bool HEAT = false>
__global__ __launch_bounds__(256) void k_kinematic_step(gptr<double> wh_row, gptr<double> wt_row, gptr<double> volr, gptr<const double> er_old,
                                                        gptr<double> er_new, gptr<const double> par, gptr<const double> area,
                                                        gptr<const int32_t> up, gptr<const double> qsur, gptr<const double> qsub,
                                                        gptr<double> qout, gptr<double> qout_sum, int64_t ncells, int64_t cld, double dts,
                                                        double dnsub, FloodRows<FLOOD> fl, DamRows<DAM> dm, HeatRows<HEAT> ht)
{
  static_assert(!(HEAT && (FLOOD || DAM)), "the heat excludes the inundation and the reservoirs");
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  int32_t u[NPAD];
#pragma unroll
  for (int p = 0; p < NPAD; p++) u[p] = up[(int64_t)p * cld + c];
  const double er = er_old[c];
  double eu[NPAD];
#pragma unroll
  for (int p = 0; p < NPAD; p++) eu[p] = er_old[u[p] >= 0 ? (int64_t)u[p] : c];
  [[maybe_unused]] double fh = 0.0;
  if constexpr (HEAT) {  // H4's gathers, in flight with K5's
    double hu[NPAD];
#pragma unroll
    for (int p = 0; p < NPAD; p++) hu[p] = ht.hr_old[u[p] >= 0 ? (int64_t)u[p] : c];
#pragma unroll
    for (int p = 0; p < NPAD; p++)
      if (u[p] >= 0) fh = fh + hu[p];
  }
  const double wh = wh_row[c], wt = wt_row[c], v = volr[c], ar = area[c], qs = qsur[c], qb = qsub[c];
  double qacc = 0.0;
  if constexpr (!FIRST) qacc = qout[c];
  const double eh = kw_hill(wh, ar, par[KW_CH * cld + c], dts);
  const double et = kw_chan(wt, par[KW_TLEN * cld + c], par[KW_TWIDTH * cld + c], par[KW_CT * cld + c], dts);
  double fin = 0.0;
#pragma unroll
  for (int p = 0; p < NPAD; p++)
    if (u[p] >= 0) fin = fin + eu[p];
  route_st(wh_row + c, wh + (qs - eh) * dts);
  route_st(wt_row + c, wt + ((eh - et) + qb) * dts);
  double en = er;
  [[maybe_unused]] double cap = 0.0;
  if constexpr (DAM) {
    cap = dm.tab[DAM_CAP * cld + c];
#ifdef ELMK_DAM_REEVAL
    if (cap > 0.0) en = kw_chan(v, par[KW_RLEN * cld + c], par[KW_RWIDTH * cld + c], par[KW_CR * cld + c], dts);
#else
    if (cap > 0.0) en = dm.rows[DAM_ENAT * cld + c];  // D4: er is what left the dam, en what left the channel
#endif
  }
  double vn = v + ((fin - en) + et) * dts;
  if constexpr (FLOOD) {
    const double vc = fl.tab[FP_VC * cld + c];
    double wf = fl.rows[FP_WF * cld + c], h = 0.0, f = 0.0;
    if (wf > 0.0 || vn > vc) {  // I1
      fp_exchange(vn, wf, h, f, vc, ar, fl.tab, cld, c);
      route_st(fl.rows + (FP_WF * cld + c), wf);
    }
    if constexpr (LAST) {
      route_st(fl.rows + (FP_DEPTH * cld + c), h);
      route_st(fl.rows + (FP_FRAC * cld + c), f);
    }
  }
  if (vn != vn) vn = __builtin_nan("");
  volr[c] = vn;
  [[maybe_unused]] double trn = 0.0;
  if constexpr (HEAT) {  // H3 - H6
    const double tt = ht.rows[HT_TT * cld + c], tr = ht.rows[HT_TR * cld + c], ho = ht.hr_old[c];
    const HeatCell x{ht.rows[HT_RAD * cld + c], ht.rows[HT_KE * cld + c], ht.rows[HT_EMS * cld + c],
                     ht.rows[HT_TA * cld + c],  ht.rows[HT_QA * cld + c], ht.rows[HT_PA * cld + c]};
    const double tsur = ht.rows[HT_TSUR * cld + c], tsub = ht.rows[HT_TSUB * cld + c];
    const double hin = ht.rows[HT_HIN * cld + c], hsrf = ht.rows[HT_HSRF * cld + c], hadj = ht.rows[HT_HADJ * cld + c],
                 hout = ht.rows[HT_HOUT * cld + c];
    const double at = par[KW_TLEN * cld + c] * par[KW_TWIDTH * cld + c], achn = par[KW_RLEN * cld + c] * par[KW_RWIDTH * cld + c];  // H0
    const double wmint = at * HT_DMIN, wminr = achn * HT_DMIN;
    const double teq = heat_fl(x.ta);
    const double gb = qb > 0.0 ? qb * tsub : qb * tt;  // H3
    const double sxt = wt > wmint ? at * heat_phi(tt, x) : 0.0;
    const double hi = eh * tsur + gb;
    const double h_t = tt * wt + ((hi - et * tt) + sxt) * dts;
    const double wtn = wt + ((eh - et) + qb) * dts;
    double adjt, adjr;
    const double ttn = heat_settle(h_t, wtn, wmint, teq, adjt);
    const double sxr = v > wminr ? achn * heat_phi(tr, x) : 0.0;  // H4
    const double h_r = tr * v + (((fh - ho) + et * tt) + sxr) * dts;
    trn = heat_settle(h_r, vn, wminr, teq, adjr);
    route_st(ht.rows + (HT_TT * cld + c), ttn);
    route_st(ht.rows + (HT_TR * cld + c), trn);
    route_st(ht.rows + (HT_HIN * cld + c), hin + hi * dts);  // H6
    route_st(ht.rows + (HT_HSRF * cld + c), hsrf + (sxt + sxr) * dts);
    route_st(ht.rows + (HT_HADJ * cld + c), hadj + (adjt + adjr));
    route_st(ht.rows + (HT_HOUT * cld + c), hout + ho * dts);
    if constexpr (LAST) route_st(ht.rows + (HT_HEAT * cld + c), ttn * wtn + trn * vn);
  }
  qacc = qacc + er;
  if constexpr (LAST) {
    const double mean = qacc / dnsub;
    route_st(qout + c, mean);
    route_st(qout_sum + c, qout_sum[c] + mean);
  } else {
    route_st(qout + c, qacc);
    double e = kw_chan(vn, par[KW_RLEN * cld + c], par[KW_RWIDTH * cld + c], par[KW_CR * cld + c], dts);
    if constexpr (DAM)
      if (cap > 0.0) e = dam_regulate(e, dm.rows[DAM_RES * cld + c], dm.rows[DAM_KRLS * cld + c], cap, dam_time(dm) & 15, dm, cld, c, dts);
    er_new[c] = e;
    if constexpr (HEAT) route_st(ht.hr_new + c, e * trn);
  }
}

// C2: one sum per dam, over the inverse map - a CSR over the dam list whose terms (cell, share) lie in CSR order.  The shape is
// k_irrigation_supply's: a workgroup takes CMD_DAMS consecutive dams, whose terms are one contiguous span.  It walks the span in tiles of
// CMD_TILE terms; every thread forms the product share * WANT[cell] of its share of a tile - coalesced loads of the terms' cell and share,
// a gather of WANT that is coalesced where a dam's dependents are neighbours - into an LDS tile, then lane t adds dam t's products out of
// LDS in CSR order.  A product is one rounding whichever lane forms it and every sum is taken by one lane in term order: the numpy
// restatement's bits, no atomics, and a dam with thousands of dependents has its loads spread over the workgroup.  CMD_DAMS = 64 and
// CMD_TILE = 1024, SUP_CELLS' and SUP_TILE's reasons: a command area holds a handful of cells up to a few thousand, so a span of 64 dams
// is mostly one or two tile passes, and the 8 KiB tile leaves the occupancy to the registers.  A dam without terms writes nothing (C0).
namespace {
constexpr int CMD_THREADS = 256, CMD_DAMS = 64, CMD_TILE = 1024;
static_assert(CMD_DAMS < CMD_THREADS && CMD_TILE % CMD_THREADS == 0, "thread t <= CMD_DAMS loads ptr; whole passes over a tile");
}  // namespace

__global__ __launch_bounds__(CMD_THREADS) void k_command_allot(gptr<const int32_t> dams, gptr<const int64_t> ptr, gptr<const int32_t> tcell,
                                                               gptr<const double> tshare, gptr<const double> want, gptr<double> res,
                                                               gptr<const double> smin, gptr<double> give, gptr<double> ratio, int64_t ndams)
{
  __shared__ double tile[CMD_TILE];
  __shared__ int64_t sp[CMD_DAMS + 1];
  const int t = threadIdx.x;
  const int64_t d0 = (int64_t)blockIdx.x * CMD_DAMS;
  const int64_t d1 = d0 + CMD_DAMS < ndams ? d0 + CMD_DAMS : ndams;
  const int nd = (int)(d1 - d0);
  if (t <= nd) sp[t] = ptr[d0 + t];
  __syncthreads();
  const int64_t P0 = sp[0], P1 = sp[nd];
  int64_t p0 = 0, p1 = 0;
  if (t < nd) {
    p0 = sp[t];
    p1 = sp[t + 1];
  }
  double W = 0.0;
  for (int64_t base = P0; base < P1; base += CMD_TILE) {
    const int m = (int)(P1 - base < CMD_TILE ? P1 - base : CMD_TILE);
#pragma unroll
    for (int k = 0; k < CMD_TILE / CMD_THREADS; k++) {
      const int q = k * CMD_THREADS + t;
      if (q < m) tile[q] = tshare[base + q] * want[tcell[base + q]];
    }
    __syncthreads();
    const int64_t lo = p0 > base ? p0 : base, hi = p1 < base + m ? p1 : base + m;
    for (int64_t p = lo; p < hi; p++) {
      const double x = tile[p - base];
      W = p == p0 ? x : W + x;
    }
    __syncthreads();
  }
  if (t < nd && p1 > p0) {
    const int64_t c = dams[d0 + t];
    const double r = res[c];
    const double a = r - smin[c];
    const double avail = a > 0.0 ? a : 0.0;
    const double rat = W > avail ? avail / W : 1.0;
    const double G = W * rat;
    route_st(res + c, r - G);
    route_st(give + c, G);
    route_st(ratio + c, rat);
  }
}

// C3: one thread per cell, a plain gather over the cells' ELL rows; every slot's loads are issued before the sum, an empty slot reads the
// cell's own RATIO and adds nothing.  A cell without a filled slot returns after its first load.
__global__ __launch_bounds__(256) void k_command_take(gptr<const int32_t> dam, gptr<const double> share, gptr<const double> want,
                                                      gptr<const double> ratio, gptr<double> take, gptr<double> qin, gptr<const double> qsur,
                                                      gptr<double> qsub, int64_t ncells, int64_t cld, double dt)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  int32_t d[CMD_NDEP];
#pragma unroll
  for (int k = 0; k < CMD_NDEP; k++) d[k] = dam[(int64_t)k * cld + c];
  if (d[0] < 0) return;  // C0
  const double wv = want[c];
  double sh[CMD_NDEP], rt[CMD_NDEP];
#pragma unroll
  for (int k = 0; k < CMD_NDEP; k++) {
    sh[k] = share[(int64_t)k * cld + c];
    rt[k] = ratio[d[k] >= 0 ? (int64_t)d[k] : c];
  }
  double got = 0.0;
#pragma unroll
  for (int k = 0; k < CMD_NDEP; k++) {
    const double x = (sh[k] * wv) * rt[k];
    if (d[k] >= 0) got = k == 0 ? x : got + x;
  }
  route_st(take + c, got);
  double q = qin[c] + got / dt;
  if (q != q) q = __builtin_nan("");
  qin[c] = q;
  route_st(qsub + c, q - qsur[c]);
}

namespace {
DamRows<true> dam_rows(const DamArgs& Dm, double dt)
{
  return DamRows<true>{(gptr<double>)Dm.rows, (gptr<const double>)Dm.tab, (gptr<const int32_t>)Dm.mstart, Dm.run, Dm.cursor, Dm.time, dt};
}
}  // namespace

void launch_routing_outlet_row(const int32_t* down, const double* src, double* dst, int64_t ncells, hipStream_t st)
{
  if (ncells <= 0) return;
  hipLaunchKernelGGL(k_routing_outlets, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, (gptr<const int32_t>)down,
                     (gptr<const double>)src, (gptr<double>)dst, ncells);
}

namespace {
// hr_old / hr_new: the buffers of this launch (the K1 launch writes hr_new only)
HeatRows<true> heat_rows(const HeatArgs& H, const double* hr_old, double* hr_new)
{
  HeatRows<true> h{};
  h.rows = (gptr<double>)H.rows;
  h.ksw = (gptr<const double>)H.ksw;
  for (int k = 0; k < HTF_N; k++) h.f[k] = H.fields[k];
  h.dtype = H.dtype;
  h.ld = H.ld;
  h.tsub_off = (int64_t)(5 + H.sublev) * H.ld;
  h.ems0 = (0.97 * 5.67e-8) / 4188000.0;  // H0: (EMIS * SB) / RHOCP
  h.hr_old = (gptr<const double>)hr_old;
  h.hr_new = (gptr<double>)hr_new;
  return h;
}
}  // namespace

void launch_routing_kinematic(const RouteArgs& A, const KinematicArgs& K, const FloodArgs& F, const DamArgs& Dm, const HeatArgs& H,
                              const OGridMap& M, const double* qrunoff, const double* qirr, const double* qsurf, const double* qh2osfc,
                              double dt, hipStream_t st, const LandArgs& Ln, const CmdArgs& Cm)
{
  if (A.ncells <= 0) return;
  const double dts = dt / (double)A.nsub;  // K0
  double *src = K.rows + KW_ER_A * A.cld, *dst = K.rows + KW_ER_B * A.cld;
  // (the heat flows go through their own two buffers in step with er's; null while the heat is off)
  double *hsrc = H.rows ? H.rows + HT_HR_A * A.cld : nullptr, *hdst = H.rows ? H.rows + HT_HR_B * A.cld : nullptr;
  const dim3 grid((unsigned)((A.ncells + 255) / 256)), block(256);
  // the DAM form of both kernels exactly while the reservoirs' rows are there, the HEAT form exactly while the heat's are (the entry
  // points keep the heat apart from the reservoirs and the inundation, and only that form is instantiated)
  with_bool(Dm.rows != nullptr, [&](auto dam) {
    with_bool(qirr != nullptr, [&](auto withdraw) {
      with_bool(H.rows != nullptr, [&](auto heat) {
        // (the LAND form exactly while the infiltration's rows and the floodplain's are there; the entry points keep it apart from the heat)
        with_bool(Ln.qland != nullptr && F.rows != nullptr, [&](auto land) {
          // (the CMD form exactly while the command areas' rows are there; the entry points keep them to the withdrawal and the reservoirs)
          with_bool(Cm.rows != nullptr, [&](auto cmd) {
            constexpr bool WITHDRAW = decltype(withdraw)::value;
            constexpr bool DAM = decltype(dam)::value, HEAT = decltype(heat)::value && !DAM, LAND = decltype(land)::value && !HEAT;
            constexpr bool CMD = decltype(cmd)::value && WITHDRAW && DAM;
            DamRows<DAM> dm;
            if constexpr (DAM) dm = dam_rows(Dm, dt);
            HeatRows<HEAT> ht;
            if constexpr (HEAT) ht = heat_rows(H, nullptr, hsrc);
            LandRows<LAND> ln;
            if constexpr (LAND) ln = LandRows<true>{(gptr<const double>)Ln.qdrain, (gptr<double>)(F.rows + FP_WF * A.cld), (gptr<double>)Ln.qland, dt};
            const auto args = [&](auto&& launch) {
              launch((gptr<const int64_t>)M.ptr, (gptr<const int32_t>)M.col, (gptr<const double>)M.w, (gptr<const double>)qrunoff,
                     (gptr<const double>)qirr, (gptr<const double>)qsurf, (gptr<const double>)qh2osfc, (gptr<const double>)A.area,
                     (gptr<const double>)(A.rows + ROUTE_VOLR * A.cld), (gptr<const double>)K.par, (gptr<double>)(A.rows + ROUTE_QIN * A.cld),
                     (gptr<double>)(K.rows + KW_QSUR * A.cld), (gptr<double>)(K.rows + KW_QSUB * A.cld), (gptr<double>)src, A.ncells, A.cld, dts);
            };
            if constexpr (CMD) {
              const CmdRows<true> cm{(gptr<const int32_t>)Cm.dam, (gptr<double>)(Cm.rows + CMD_WANT * A.cld)};
              args([&](auto... a) { hipLaunchKernelGGL((k_kinematic_prep_cmd<LAND>), grid, block, 0, st, a..., dm, ln, cm); });
            } else {
              args([&](auto... a) { hipLaunchKernelGGL((k_kinematic_prep<WITHDRAW, DAM, HEAT, LAND>), grid, block, 0, st, a..., dm, ht, ln); });
            }
          });
        });
      });
    });
  });
  if (Cm.rows && Dm.rows && qirr) {  // C2, C3: between the K1 launch and the first sub-step
    if (Cm.ndams > 0)
      hipLaunchKernelGGL(k_command_allot, dim3((unsigned)((Cm.ndams + CMD_DAMS - 1) / CMD_DAMS)), dim3(CMD_THREADS), 0, st,
                         (gptr<const int32_t>)Cm.dams, (gptr<const int64_t>)Cm.ptr, (gptr<const int32_t>)Cm.tcell, (gptr<const double>)Cm.tshare,
                         (gptr<const double>)(Cm.rows + CMD_WANT * A.cld), (gptr<double>)(Dm.rows + DAM_RES * A.cld),
                         (gptr<const double>)(Dm.tab + DAM_SMIN * A.cld), (gptr<double>)(Cm.rows + CMD_GIVE * A.cld),
                         (gptr<double>)(Cm.rows + CMD_RATIO * A.cld), Cm.ndams);
    hipLaunchKernelGGL(k_command_take, grid, block, 0, st, (gptr<const int32_t>)Cm.dam, (gptr<const double>)Cm.share,
                       (gptr<const double>)(Cm.rows + CMD_WANT * A.cld), (gptr<const double>)(Cm.rows + CMD_RATIO * A.cld),
                       (gptr<double>)(Cm.rows + CMD_TAKE * A.cld), (gptr<double>)(A.rows + ROUTE_QIN * A.cld),
                       (gptr<const double>)(K.rows + KW_QSUR * A.cld), (gptr<double>)(K.rows + KW_QSUB * A.cld), A.ncells, A.cld, dt);
  }
  for (int s = 0; s < A.nsub; s++) {
    const auto args = [&](auto&& launch) {
      launch((gptr<double>)(K.rows + KW_WH * A.cld), (gptr<double>)(K.rows + KW_WT * A.cld), (gptr<double>)(A.rows + ROUTE_VOLR * A.cld),
             (gptr<const double>)src, (gptr<double>)dst, (gptr<const double>)K.par, (gptr<const double>)A.area, (gptr<const int32_t>)A.up,
             (gptr<const double>)(K.rows + KW_QSUR * A.cld), (gptr<const double>)(K.rows + KW_QSUB * A.cld),
             (gptr<double>)(A.rows + ROUTE_QOUT * A.cld), (gptr<double>)(A.rows + ROUTE_QOUT_SUM * A.cld), A.ncells, A.cld, dts, (double)A.nsub);
    };
    // (I6: the same launch in the flood form)
    with_bool(F.rows != nullptr, [&](auto flood) {
      with_npad(A.npad, [&](auto npad) {
        with_bool(s == 0, [&](auto first) {
          with_bool(s == A.nsub - 1, [&](auto last) {
            with_bool(Dm.rows != nullptr, [&](auto dam) {
              with_bool(H.rows != nullptr, [&](auto heat) {
                constexpr int NPAD = decltype(npad)::value;
                constexpr bool FIRST = decltype(first)::value, LAST = decltype(last)::value;
                constexpr bool FLOOD = decltype(flood)::value, DAM = decltype(dam)::value;
                // (H: the entry points keep the heat apart from the inundation and the reservoirs)
                constexpr bool HEAT = decltype(heat)::value && !FLOOD && !DAM;
                FloodRows<FLOOD> fl;
                if constexpr (FLOOD) fl = FloodRows<true>{(gptr<double>)F.rows, (gptr<const double>)F.tab};
                DamRows<DAM> dm;
                if constexpr (DAM) dm = dam_rows(Dm, dts * (double)A.nsub);
                HeatRows<HEAT> ht;
                if constexpr (HEAT) ht = heat_rows(H, hsrc, hdst);
                args([&](auto... a) {
                  hipLaunchKernelGGL((k_kinematic_step<NPAD, FIRST, LAST, FLOOD, DAM, HEAT>), grid, block, 0, st, a..., fl, dm, ht);
                });
              });
            });
          });
        });
      });
    });
    double* const t = src;
    src = dst;
    dst = t;
    double* const th = hsrc;
    hsrc = hdst;
    hdst = th;
  }
}

}  // namespace elmk
