// k_soil_hydrology.hip - column soil hydrology on the device (elmk_soil_hydrology_*; ELM v1's SoilHydrologyMod in the CLM4.5
// formulation): surface runoff, infiltration with the h2osfc store, the Zeng-Decker Richards solve, the water-table update and
// drainage.  The reference has none of it (driver/kokkos/conserved_quantity_kokkos.cc:22 hardwires hydrology_source_sink = 0.0): it
// expects an external subsurface model.  The operation is stated in include/elmk.h "soil hydrology", sections A - H, and restated on
// the host in elmkernels_amd/hydrology.py: column(); this file follows that function statement by statement, and the two agree bit
// for bit.  No contraction (the Makefile's -ffp-contract=off), `/` the correctly rounded fp64 division, dmin / dmax the written-out
// comparisons, pow and exp the glibc restatements elmk_pow / elmk_exp.
//
// One launch, one thread per column, 256-thread workgroups, every access a coalesced SoA row.  Every loop over the ten layers is
// fully unrolled and every per-layer array is indexed by compile-time constants only, so the arrays live in registers: where the
// operation indexes by the water-table layer jwt (the recharge, the walks of the water table) the loop runs over all layers under a
// predicate instead.  Each state row is read once and written once; the byte tally per column is in
// DESIGN.md section 20.
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_math.h"

namespace elmk {

namespace {
constexpr int HN = ELMK_HYD_NLAYER;  // hydrologically active layers: layer j is level NLEVSNO + j
static_assert(HN == 10 && NLEVSNO + HN + 1 <= NLEVTOT + 1 && HN <= NLEVGRND, "ten layers above the bedrock layers");
constexpr double HY_DENH2O = 1000.0, HY_DENICE = 917.0, HY_E_ICE = 6.0, HY_SMPMIN = -1.0e8, HY_WATMIN = 0.01;
constexpr double HY_PC = 0.4, HY_MU = 0.13889, HY_FFF_S = 0.5, HY_FFF_D = 2.5, HY_AQUIFER_MAX = 5000.0, HY_ROUS_MIN = 0.02;
constexpr double HY_TFRZ = 273.15, HY_SAT_LEV = 0.9;  // F': the frost table and the perched water table

__device__ __forceinline__ double hy_sy(double zwt, double watsat, double sucsat, double bsw)
{
  return dmax(HY_ROUS_MIN, watsat * (1.0 - elmk_pow(1.0 + (1.0e3 * zwt) / sucsat, -1.0 / bsw)));
}
__device__ __forceinline__ double hy_canon(double x) { return x != x ? __builtin_nan("") : x; }
}  // namespace

// The rows a launch is handed: the feature's, and in the frost form the extension's.  The plain form keeps the kernel arguments it had
// before the extension existed, so that its code is that kernel's, instruction for instruction.
template <bool FROST, bool ROF = false> struct HydRows {
  gptr<double> rows;
};
template <> struct HydRows<true, false> {
  gptr<double> rows, frows;
};
// ROF: the floodplain infiltration (include/elmk.h "floodplain infiltration", F1 - F3): the column's cell, the routing's WF, FLOOD_FRAC and
// area rows over the cells, and the extension's three column rows [ELMK_FPI_NROWS][ld]
struct RofRows {
  gptr<const int32_t> cellof;
  gptr<const double> wf, ff, area;
  gptr<double> out;
};
template <> struct HydRows<false, true> {
  gptr<double> rows;
  RofRows rof;
};
template <> struct HydRows<true, true> {
  gptr<double> rows, frows;
  RofRows rof;
};
// LAT: the hillslope lateral flow (include/elmk.h "hillslope lateral flow", L3): the extension's QLAT_NET row [ld] and down [ld]
struct LatRows {
  gptr<double> rows;
  gptr<const double> qnet;
  gptr<const int32_t> down;
};

// FROST: the F' form of the drainage (elmk_soil_hydrology_frost_enable), frows its ELMK_HYDF_NROWS rows.  It keeps nothing of its own
// live across D and E: the ten temperatures are loaded at F'.0 and reduced at once to kf and frozen, and hksat[j] and the node depths of
// kf, kp and kp + 1 are loaded again where they are needed.  It also loads dz and the ice again at F' and evaluates effpor and icefrac
// from them a second time, which frees their registers during the solve: with them carried the kernel spilled to scratch (DESIGN.md
// section 20).  Branches A and B share one conductivity sum and one removal walk: they differ in the layers and in which table the
// walk moves.
// ROF: F1 - F3 at the end of C.  The column's cell and the cell's three values are loaded there, through an index the compiler cannot
// match with the loads at the top, and the three rows are stored there: nothing of the form is live into D.
// LAT: L3 in the place of F.1's rsub_top.  down[c] and QLAT_NET[c] are loaded at F through a laundered index, as the other forms' rows
// are: nothing of the form is live across D and E.  A column with down == -2 runs F.1 as it stands.
// The LAT form is a kernel of its own name, k_soil_hydrology_lat, so that the four forms of k_soil_hydrology keep their names, their
// arguments and their code.  The two kernels share one body, k_soil_hydrology_body.h, included into each: as a device function that both
// call, the inliner left the four old forms with other register counts than they had.
template <bool FROST, bool ROF>
__global__ __launch_bounds__(256) void k_soil_hydrology(const DevState* __restrict__ S, HydRows<FROST, ROF> R, double dt)
{
  constexpr bool LAT = false;
#include "k_soil_hydrology_body.h"
}
// the LAT form (FROST = false, ROF = false, LAT = true); a template over its rows so that the other forms' statements are discarded
template <class ROWS>
__global__ __launch_bounds__(256) void k_soil_hydrology_lat(const DevState* __restrict__ S, ROWS R, double dt)
{
  constexpr bool FROST = false, ROF = false, LAT = true;
#include "k_soil_hydrology_body.h"
}

// The plain form first in the unit's code object, where the kernel stood before the extension: with the frost form in front of it the
// same instructions ran 1 % slower on the thawed tier.
template __global__ void k_soil_hydrology<false, false>(const DevState* __restrict__, HydRows<false, false>, double);
template __global__ void k_soil_hydrology<true, false>(const DevState* __restrict__, HydRows<true, false>, double);
template __global__ void k_soil_hydrology<false, true>(const DevState* __restrict__, HydRows<false, true>, double);
template __global__ void k_soil_hydrology<true, true>(const DevState* __restrict__, HydRows<true, true>, double);
template __global__ void k_soil_hydrology_lat<LatRows>(const DevState* __restrict__, LatRows, double);

void launch_soil_hydrology(const DevState* S, int64_t n, double* rows, double* frost_rows, double dt, hipStream_t st, const RofArgs* rof,
                           const LatArgs* lat)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (lat) {  // (the host API keeps the frost table and the floodplain infiltration off while the lateral flow is on)
    hipLaunchKernelGGL((k_soil_hydrology_lat<LatRows>), grid, block, 0, st, S, LatRows{(gptr<double>)rows, (gptr<const double>)lat->qnet, (gptr<const int32_t>)lat->down}, dt);
    return;
  }
  if (rof) {
    const RofRows r{(gptr<const int32_t>)rof->cellof, (gptr<const double>)rof->wf, (gptr<const double>)rof->ff, (gptr<const double>)rof->area,
                    (gptr<double>)rof->out};
    if (frost_rows)
      hipLaunchKernelGGL((k_soil_hydrology<true, true>), grid, block, 0, st, S, HydRows<true, true>{(gptr<double>)rows, (gptr<double>)frost_rows, r}, dt);
    else hipLaunchKernelGGL((k_soil_hydrology<false, true>), grid, block, 0, st, S, HydRows<false, true>{(gptr<double>)rows, r}, dt);
    return;
  }
  if (frost_rows)
    hipLaunchKernelGGL((k_soil_hydrology<true, false>), grid, block, 0, st, S, HydRows<true, false>{(gptr<double>)rows, (gptr<double>)frost_rows}, dt);
  else hipLaunchKernelGGL((k_soil_hydrology<false, false>), grid, block, 0, st, S, HydRows<false, false>{(gptr<double>)rows}, dt);
}

}  // namespace elmk
