// k_irrigation.hip - irrigation on the device (elmk_irrigation_*; include/elmk.h "irrigation"): ELM's daily demand check (CLM4.5 / ELM v1
// CanopyFluxes; the reference keeps it as a comment block, src/physics/canopy_fluxes_impl.hh:17-91) and the application of
// canopy_hydrology's Irrigation() and ground_flux (src/physics/canopy_hydrology_impl.hh:70-80, :105-118), which the reference never
// reaches: it hardwires irrig_rate, n_irrig_steps_left and qflx_irrig to zero.  One launch between the seven wrappers and
// soil_temperature.  elmkernels_amd/irrigation.py: step() restates the operation in numpy, and this file follows it statement by
// statement.  No contraction (the Makefile's -ffp-contract=off), plain IEEE comparisons, `/` the correctly rounded fp64 division,
// elmk_pow; a NaN is stored into a row as the canonical quiet NaN.
//
// One thread per column, 256-thread workgroups, every access a coalesced SoA row, no LDS.  A column that neither applies nor checks
// reads sched, NLEFT, btran, elai and frac_veg_nosno (4 + 8 + 8 + 8 + 4 bytes in the fp64 build) and writes QFLX_IRRIG (8).  A column
// that applies reads RATE and do_capsnow as well and updates NLEFT and one state field.  Only a column whose local clock passes 06:00
// in this step walks the soil levels: each level loads in program order and the lane leaves the loop at its first frozen level, as
// k_active_layer does; sched is the longitude, so on a spatially numbered domain these columns are neighbours and whole waves skip the
// walk.  The unit carries no nontemporal hint: none has been measured for it.
#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

namespace {
constexpr int IRR_NSOIL = NLEVGRND;  // soil layers 0 .. 14 are levels NLEVSNO + j
static_assert(NLEVSNO == 5 && NLEVGRND == 15 && NLEVSNO + NLEVGRND <= NLEVTOT, "level 5 + j is soil layer j, j = 0 .. 14");
constexpr double IRR_FACTOR = 0.7;             // irrig_factor
constexpr double IRR_MIN_LAI = 0.0;            // irrig_min_lai
constexpr double IRR_BTRAN_THRESH = 0.999999;  // irrig_btran_thresh
constexpr int IRR_START = 21600, IRR_DAY = 86400;  // 06:00 local time; the window's 14400 s are in nspd

__device__ __forceinline__ void irr_st(gptr<double> p, double v)
{
  if (v != v) v = __builtin_nan("");
  *p = v;
}
}  // namespace

#define LV(f, lev) S->f[(int64_t)(lev) * ld + c]

// RUN: tod from the pad word of the step's row of the device step table (elmk_run); otherwise the argument (elmk_irrigation)
template <bool RUN>
__global__ __launch_bounds__(256) void k_irrigation(const DevState* __restrict__ S, gptr<double> irr, gptr<const int32_t> sched, int idt,
                                                    int nspd, int tod, const RunRow* __restrict__ rows,
                                                    const int32_t* __restrict__ cursor)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  if constexpr (RUN) tod = (rows[*cursor].pad >> RUN_PAD_TOD_SHIFT) & RUN_PAD_TOD_MASK;  // (above it: the reservoirs' month)
  const gptr<double> rate_p = irr + (int64_t)ELMK_IRR_RATE * ld + c, nleft_p = irr + (int64_t)ELMK_IRR_NLEFT * ld + c,
                     qirr_p = irr + (int64_t)ELMK_IRR_QFLX_IRRIG * ld + c;

  // what every column reads, issued together
  const int32_t sc = sched[c];
  const double n = *nleft_p;
  const int fvn = S->frac_veg_nosno[c];
  const double elai = S->elai[c], btran = S->btran[c];

  // A: apply
  double q = 0.0;
  if (n > 0.0) {
    q = *rate_p;
    *nleft_p = n - 1.0;
  }
  irr_st(qirr_p, q);
  if (q > 0.0) {
    if (S->do_capsnow[c]) S->qflx_snwcp_liq[c] += q;
    else S->qflx_rain_grnd[c] += q;
  }

  // B: check
  if (!(sc >= 0 && fvn != 0 && elai > IRR_MIN_LAI && btran < IRR_BTRAN_THRESH)) return;
  const int local = (tod + sc) % IRR_DAY;
  const int since = (local - IRR_START + IRR_DAY) % IRR_DAY;
  if (!(since < idt)) return;
  const int vtype = S->vtype[c];
  const double smpso = (unsigned)vtype < (unsigned)ELMK_MXPFT ? S->pft_psn[vtype][P_smpso] : __builtin_nan("");  // (never outside the table)
  const double dtn = (double)idt * (double)nspd;
  double rate = 0.0;
  for (int j = 0; j < IRR_NSOIL; j++) {
    const double t = LV(t_soisno, NLEVSNO + j);
    if (t <= TFRZ) break;
    const double rf = LV(rootfr, j);
    if (rf > 0.0) {
      const double effpor = LV(eff_porosity, j), dzj = LV(dz, NLEVSNO + j);
      const double vol_liq_so = effpor * elmk_pow(-smpso / (double)LV(sucsat, j), -1.0 / (double)LV(bsw, j));
      const double liq_so = vol_liq_so * DENH2O * dzj;
      const double liq_sat = effpor * DENH2O * dzj;
      const double deficit = dmax((liq_so + IRR_FACTOR * (liq_sat - liq_so)) - (double)LV(h2osoi_liq, NLEVSNO + j), 0.0);
      rate = rate + deficit / dtn;
    }
  }
  *nleft_p = (double)nspd;
  irr_st(rate_p, rate);
}
#undef LV

template <bool RUN>
static void launch_irr(const DevState* S, int64_t n, double* rows, const int32_t* sched, int idt, int tod, const RunRow* table,
                       const int32_t* cursor, hipStream_t st)
{
  if (n <= 0) return;
  const int nspd = (14400 + (idt - 1)) / idt;
  hipLaunchKernelGGL((k_irrigation<RUN>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, (gptr<double>)rows,
                     (gptr<const int32_t>)sched, idt, nspd, tod, table, cursor);
}

void launch_irrigation(const DevState* S, int64_t n, double* rows, const int32_t* sched, int idt, int tod, hipStream_t st)
{
  launch_irr<false>(S, n, rows, sched, idt, tod, nullptr, nullptr, st);
}

void launch_irrigation_run(const DevState* S, int64_t n, double* rows, const int32_t* sched, int idt, const RunRow* table,
                           const int32_t* cursor, hipStream_t st)
{
  launch_irr<true>(S, n, rows, sched, idt, 0, table, cursor, st);
}

}  // namespace elmk
