// k_hillslope.hip - hillslope lateral flow on the device (elmk_hillslope_*; CLM5 / CTSM's SubsurfaceLateralFlow with use_hillslope,
// Swenson et al. 2019): the two launches in front of the soil hydrology kernel's LAT form.  The operation is stated in include/elmk.h
// "hillslope lateral flow", L1 and L2, and restated on the host in elmkernels_amd/hydrology.py: hillslope_head() and hillslope_flow();
// this file follows those functions statement by statement, and the two agree bit for bit.  The conventions are the hydrology's: no
// contraction (the Makefile's -ffp-contract=off), `/` the correctly rounded fp64 division, dmin / dmax the written-out comparisons, pow
// the glibc restatement elmk_pow.
//
// k_hillslope_head (L1): one thread per column, every access a coalesced SoA row; writes HEAD and TRANS.
// k_hillslope_flow<NPAD> (L2): one thread per column; gathers HEAD and TRANS of the downhill column and of up to NPAD uphill columns
// through the host-checked map (elmk_maps.h: hillslope_check - every index it holds lies in [0, ncols)).  Written by one launch,
// gathered by the next: no atomics, no LDS.  Each edge's flux is evaluated by both of its ends from the same operands, so both hold the
// same bits.
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_math.h"

namespace elmk {

namespace {
constexpr int HN = ELMK_HYD_NLAYER;
constexpr double HS_DENICE = 917.0, HS_E_ICE = 6.0;
__device__ __forceinline__ double hs_canon(double x) { return x != x ? __builtin_nan("") : x; }

// L2: the flux of the edge out of column u, m3/s.  d = down[u] (-1: the stream); hd, td: HEAD and TRANS of d (unused for the stream)
__device__ __forceinline__ double hs_vol(int32_t d, double hu, double tu, double hd, double td, double dist, double width)
{
  double g;
  if (d == -1) g = dmax(hu / dist, 0.0);
  else g = (hu - hd) / dist;
  g = dmin(dmax(g, -2.0), 2.0);
  const double t = (d != -1 && g < 0.0) ? td : tu;
  return t * width * g;
}
}  // namespace

__global__ __launch_bounds__(256) void k_hillslope_head(const DevState* __restrict__ S, gptr<const double> hyd, gptr<const int32_t> down,
                                                        gptr<const double> elev, double k_aniso, gptr<double> rows)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  double head = 0.0, trans = 0.0;
  if (down[c] != -2) {
#define SL(f, j) S->f[(int64_t)(NLEVSNO + (j)) * ld + c]
    const double zwt = hyd[(int64_t)ELMK_HYD_ZWT * ld + c];
    double zi[HN + 1];
#pragma unroll
    for (int j = 0; j <= HN; j++) zi[j] = SL(zisoi, j);  // zi[0] = the surface, zi[j + 1] = the bottom of layer j
    int jwt = HN;
#pragma unroll
    for (int j = HN - 1; j >= 0; j--)
      if (zwt <= zi[j + 1]) jwt = j;
    if (jwt < HN) {
      const int j0 = jwt - 1 > 0 ? jwt - 1 : 0;
      double si = 0.0, sd = 0.0, t = 0.0;
#pragma unroll
      for (int j = 0; j < HN; j++) {
        const double dz = SL(dz, j);
        if (j >= j0) {
          const double watsat = S->watsat[(int64_t)j * ld + c];
          const double vol_ice = dmin(watsat, (double)SL(h2osoi_ice, j) / (dz * HS_DENICE));
          const double icefrac = dmin(1.0, vol_ice / watsat);
          const double dzmm = dz * 1.0e3;
          si = si + icefrac * dzmm;
          sd = sd + dzmm;
        }
        if (j >= jwt) t = t + hyd[(int64_t)(ELMK_HYD_HKSAT + j) * ld + c] * (j == jwt ? zi[j + 1] - zwt : dz);
      }
      const double imp = elmk_pow(10.0, -HS_E_ICE * (si / sd));
      trans = imp * t * 1.0e-3 * k_aniso;
    }
    head = elev[c] - zwt;
#undef SL
  }
  rows[(int64_t)ELMK_HS_HEAD * ld + c] = hs_canon(head);
  rows[(int64_t)ELMK_HS_TRANS * ld + c] = hs_canon(trans);
}

template <int NPAD>
__global__ __launch_bounds__(256) void k_hillslope_flow(int64_t n, int64_t ld, gptr<const int32_t> down, gptr<const int32_t> up,
                                                        gptr<const double> geom, gptr<double> rows)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  gptr<const double> head = rows + (int64_t)ELMK_HS_HEAD * ld, trans = rows + (int64_t)ELMK_HS_TRANS * ld;
  gptr<const double> dist = geom + (int64_t)HS_DIST * ld, width = geom + (int64_t)HS_WIDTH * ld, area = geom + (int64_t)HS_AREA * ld;
  const int32_t d = down[c];
  double out = 0.0, in = 0.0, net = 0.0, qs = 0.0;
  if (d != -2) {
    const double hc = head[c], tc = trans[c], ac = area[c];
    double hd = 0.0, td = 0.0;
    if (d >= 0) {
      hd = head[d];
      td = trans[d];
    }
    const double vol = hs_vol(d, hc, tc, hd, td, dist[c], width[c]);
    out = 1.0e3 * vol / ac;
#pragma unroll
    for (int p = 0; p < NPAD; p++) {
      const int32_t u = up[(int64_t)p * ld + c];
      if (u >= 0) in = in + 1.0e3 * hs_vol((int32_t)c, head[u], trans[u], hc, tc, dist[u], width[u]) / ac;
    }
    net = out - in;
    if (d == -1) qs = vol;
  }
  rows[(int64_t)ELMK_HS_QLAT_OUT * ld + c] = hs_canon(out);
  rows[(int64_t)ELMK_HS_QLAT_IN * ld + c] = hs_canon(in);
  rows[(int64_t)ELMK_HS_QLAT_NET * ld + c] = hs_canon(net);
  rows[(int64_t)ELMK_HS_QSTREAM * ld + c] = hs_canon(qs);
}

void launch_hillslope(const DevState* S, int64_t n, int64_t ld, const double* hyd_rows, const HillslopeArgs& A, hipStream_t st)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_hillslope_head, grid, block, 0, st, S, (gptr<const double>)hyd_rows, (gptr<const int32_t>)A.down,
                     (gptr<const double>)(A.geom + (size_t)HS_ELEV * (size_t)ld), A.k_aniso, (gptr<double>)A.rows);
#define FLOW(NP)                                                                                                          \
  hipLaunchKernelGGL((k_hillslope_flow<NP>), grid, block, 0, st, n, ld, (gptr<const int32_t>)A.down, (gptr<const int32_t>)A.up, \
                     (gptr<const double>)A.geom, (gptr<double>)A.rows)
  switch (A.npad) {
    case 1: FLOW(1); break;
    case 2: FLOW(2); break;
    case 4: FLOW(4); break;
    default: FLOW(8); break;
  }
#undef FLOW
}

}  // namespace elmk
