// k_active_layer.hip - active layer thickness on the device (elmk_active_layer_*; ELM's ActiveLayerMod::alt_calc): the depth of the
// thaw front of every column, its running annual maximum and last year's maximum, with the layer indices altmax_indx and
// altmax_lastyear_indx that normalize_unfrozen_rootfr reads every step (soil_moist_stress_impl.hh:41).  The reference marks the two
// index fields NEED!! (src/data/elm_state_impl.hh:274-276) and has no alt_calc; this is ELM's routine, run once per step after the
// soil temperature solve.
//
// Per column c (include/elmk.h "active layer thickness"; elmkernels_amd/active_layer.py: update restates it in numpy), with t[j] and
// z[j] the temperature and node depth of soil layer j = 0 .. 14 (level 5 + j of t_soisno / zsoi, widened to fp64), tfrz = 273.15, every
// comparison the plain IEEE `>`, no contraction, `/` the correctly rounded fp64 division:
//   if (roll_c) { altmax_lastyear = altmax; altmax_lastyear_indx = altmax_indx; altmax = +0.0; altmax_indx = -1; }
//   if (t[14] > tfrz) { a = z[14]; k = 14; }
//   else { k = the largest j in 0 .. 13 with t[j] > tfrz, or -1;
//          a = k >= 0 ? z[k] + ((t[k] - tfrz) * (z[k+1] - z[k])) / (t[k] - t[k+1]) : +0.0; }
//   if (a != a) a = the canonical quiet NaN 0x7FF8000000000000;      (IEEE leaves a NaN result's sign and payload to the implementation)
//   alt = a;  if (a > altmax) { altmax = a; altmax_indx = k; }
// roll_c = (rollover & ELMK_ALT_ROLL_NORTH) && north_c || (rollover & ELMK_ALT_ROLL_SOUTH) && !north_c, north_c = sin(lat) > 0.0 from the
// column geography (ELMK_GEO_SIN_LAT).
//
// One thread per column, 256-thread workgroups, every access a coalesced SoA row.  The search walks the soil levels from the bottom
// upward and carries the level below in a register, so t[k+1] is never re-read, and a lane leaves the loop at its first thawed
// layer: the wave leaves it once every lane has.  On columns without permafrost that is one row of t_soisno (the bottom layer is
// thawed) instead of fifteen.  zsoi is read at k and k + 1 only.  The stores of altmax and altmax_indx and, on a rollover, of the two
// last-year rows are conditional per lane; altmax is read for the compare, altmax_indx only by a lane that rolls over.  Bytes per
// column on the byte tally (fp64 state, no rollover): frozen tier 15 x 8 (t_soisno) + 8 (altmax) + 8 (alt) = 136, up to 16 + 12 more
// where a layer is found and the maximum grows; thawed tier 8 + 8 + 8 + 8 = 32, + 12 where the maximum grows.
//
// ELMK_ALT_EARLY_EXIT (default 1; 0 = every lane loads all fifteen levels and selects) and the nontemporal hint (the Makefile's
// FLAGS_k_active_layer: ELMK_STATE_NT, bit 0 loads, bit 1 stores, here applied to the rows of the feature as well as to the state
// fields) are the two switches of the A/B in tests/tools/active_layer_cost.py; DESIGN.md section 19 records what was measured.
#include "elmk_dev.h"
#include "elmk_kernels.h"

#ifndef ELMK_ALT_EARLY_EXIT
#define ELMK_ALT_EARLY_EXIT 1
#endif
#ifdef ELMK_STATE_NT
#define ELMK_ALT_NT (ELMK_STATE_NT)
#else
#define ELMK_ALT_NT 0
#endif

namespace elmk {

namespace {
constexpr double ALT_TFRZ = 273.15;
constexpr int ALT_NSOIL = NLEVGRND;  // soil layers 0 .. 14 are levels NLEVSNO + j
static_assert(NLEVSNO == 5 && NLEVGRND == 15 && NLEVSNO + NLEVGRND <= NLEVTOT, "level 5 + j is soil layer j, j = 0 .. 14");

template <typename T> __device__ __forceinline__ T alt_ld(gptr<T> p)
{
  return (ELMK_ALT_NT & 1) ? __builtin_nontemporal_load(p) : *p;
}
template <typename T> __device__ __forceinline__ void alt_st(gptr<T> p, T v)
{
  if (ELMK_ALT_NT & 2) __builtin_nontemporal_store(v, p);
  else *p = v;
}
}  // namespace

// RUN: the rollover bits from the pad word of the step's row of the device step table (elmk_run, as k_phenology_run reads its months);
// otherwise the argument (elmk_active_layer_update)
template <bool RUN>
__global__ __launch_bounds__(256) void k_active_layer(const dfield t_soisno, const dfield zsoi, gptr<int32_t> altmax_indx,
                                                      gptr<int32_t> altmax_lastyear_indx, gptr<double> alt, gptr<double> altmax,
                                                      gptr<double> altmax_lastyear, gptr<const double> sin_lat, int64_t ld,
                                                      int64_t ncols, const RunRow* __restrict__ rows,
                                                      const int32_t* __restrict__ cursor, int rollover)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  if constexpr (RUN) rollover = rows[*cursor].pad & RUN_PAD_ROLL_MASK;  // (above the mask: the irrigation's time of day)
  const dfield t = t_soisno + (int64_t)NLEVSNO * ld + c, z = zsoi + (int64_t)NLEVSNO * ld + c;

  // the search, from the bottom upward; t2 = the level below the one in hand
  int k = -1;
  double t1 = 0.0, t2 = t[(int64_t)(ALT_NSOIL - 1) * ld];
  if (t2 > ALT_TFRZ) {
    k = ALT_NSOIL - 1;
  } else {
#if ELMK_ALT_EARLY_EXIT
    for (int j = ALT_NSOIL - 2; j >= 0; j--) {
      const double tj = t[(int64_t)j * ld];
      if (tj > ALT_TFRZ) {
        k = j;
        t1 = tj;
        break;
      }
      t2 = tj;
    }
#else
    double below = t2;
#pragma unroll
    for (int j = ALT_NSOIL - 2; j >= 0; j--) {
      const double tj = t[(int64_t)j * ld];
      if (k < 0 && tj > ALT_TFRZ) {
        k = j;
        t1 = tj;
        t2 = below;
      }
      below = tj;
    }
#endif
  }
  double a = 0.0;
  if (k == ALT_NSOIL - 1) {
    a = z[(int64_t)k * ld];
  } else if (k >= 0) {
    const double z1 = z[(int64_t)k * ld], z2 = z[(int64_t)(k + 1) * ld];
    a = z1 + ((t1 - ALT_TFRZ) * (z2 - z1)) / (t1 - t2);
  }
  // one NaN for every way to get one: the sign and payload an operation gives a NaN differ between this device (a negated operand
  // flips the sign of a NaN it carries) and the host
  if (a != a) a = __builtin_nan("");

  // the annual rollover comes before the compare (ELM's order); sin_lat is read only in a step that rolls a hemisphere over
  bool roll = false;
  if (rollover != 0) {
    const bool north = sin_lat[c] > 0.0;
    roll = north ? (rollover & ELMK_ALT_ROLL_NORTH) != 0 : (rollover & ELMK_ALT_ROLL_SOUTH) != 0;
  }
  double am = alt_ld(altmax + c);
  if (roll) {
    alt_st(altmax_lastyear + c, am);
    alt_st(altmax_lastyear_indx + c, alt_ld(altmax_indx + c));
    am = 0.0;
  }
  alt_st(alt + c, a);
  if (a > am) {
    alt_st(altmax + c, a);
    alt_st(altmax_indx + c, (int32_t)k);
  } else if (roll) {
    alt_st(altmax + c, 0.0);
    alt_st(altmax_indx + c, (int32_t)-1);
  }
}

template <bool RUN>
static void launch_alt(const ActiveLayerArgs& A, const RunRow* rows, const int32_t* cursor, int rollover, hipStream_t st)
{
  if (A.ncols <= 0) return;
  hipLaunchKernelGGL((k_active_layer<RUN>), dim3((unsigned)((A.ncols + 255) / 256)), dim3(256), 0, st,
                     field_of<ELMK_F64>::from(A.t_soisno), field_of<ELMK_F64>::from(A.zsoi), (gptr<int32_t>)A.altmax_indx,
                     (gptr<int32_t>)A.altmax_lastyear_indx, (gptr<double>)A.rows, (gptr<double>)(A.rows + A.ld),
                     (gptr<double>)(A.rows + 2 * A.ld), (gptr<const double>)A.sin_lat, A.ld, A.ncols, rows, cursor, rollover);
}

void launch_active_layer(const ActiveLayerArgs& A, int rollover, hipStream_t st) { launch_alt<false>(A, nullptr, nullptr, rollover, st); }

void launch_active_layer_run(const ActiveLayerArgs& A, const RunRow* rows, const int32_t* cursor, hipStream_t st)
{
  launch_alt<true>(A, rows, cursor, 0, st);
}

}  // namespace elmk
