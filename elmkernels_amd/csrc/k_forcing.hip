// k_forcing.hip - the per-column functors kokkos_init_timestep runs ahead of its own kernel:
//
//   get_forcing (driver/kokkos/atm_forcing_kokkos.cc:47-75): eight parallel_for launches in the reference, one per
//   forcing stream - ComputeAtmForcing_TBOT, _PBOT, _QBOT|RH, _FLDS, _FSDS, _PREC, _WIND, _ZBOT
//   (src/physics/atm_physics_impl.hh:27-245).  A column only reads what the earlier functors wrote for the SAME column
//   (tbot -> qbot, lwrad, rain/snow; pbot -> qbot, lwrad), so they are one streaming kernel here, in the wrapper's order.
//   The raw streams are the two records of AtmDataManager::data(ntimes, ncells) that bracket the model time, held as the
//   two-level state fields atm_* (level 0 = record t_idx, level 1 = t_idx + 1): already time-major, i.e. SoA.
//
//   ComputePhenology (src/physics/phenology_physics_impl.hh:22-69, run by update_phenology,
//   driver/kokkos/phenology_kokkos.cc:59-62) over the two bracketing months mlai .. mhbot.
//
// The time logic that picks t_idx and the weights (AtmDataManager::forc_t_idx_check_bounds, forcing_time_weights,
// atm_data_impl.hh:147-199) works on dates on the host and stays with the caller; the readers are file I/O.
// Algorithmic bytes per column: get_forcing 7 x 16 + 8 (coszen) read, 17 x 8 written = 256; phenology 4 x 16 + 20 read,
// 6 x 8 + 4 written = 136.
//
// Shortwave (elmk_set_shortwave_mode): every forcing kernel has a COSZEN variant (the CZ switch of get_forcing_col, 8 bytes more read
// per column: czf, the forcing interval's mean cos(zenith), k_solar.hip).  The REFERENCE kernels are the reference's as before.
//
// Downscaling (elmk_set_downscaling): every forcing kernel, COSZEN or not, has a TOPO variant (the DS switch of get_forcing_col: 16
// bytes more read per column, the column's elevation and the forcing's surface height, and 8 written while longwave groups are set,
// Lg) that adjusts the near-surface air from the forcing's height to the column's (downscale_col).  The OFF kernels are as before.
#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

#define LV(f, lev) S->f[(int64_t)(lev) * ld + c]

// atm_physics_impl.hh:205-245
__device__ __forceinline__ double interp_forcing(double wt1, double wt2, double forc1, double forc2) { return forc1 * wt1 + forc2 * wt2; }
__device__ __forceinline__ double tdc(double t) { return dmin(50.0, dmax(-50.0, (t - TFRZ))); }
__device__ __forceinline__ double esatw(double t)
{
  const double a0 = 6.107799961, a1 = 4.436518521e-01, a2 = 1.428945805e-02, a3 = 2.650648471e-04, a4 = 3.031240396e-06,
               a5 = 2.034080948e-08, a6 = 6.136820929e-11;
  return 100.0 * (a0 + t * (a1 + t * (a2 + t * (a3 + t * (a4 + t * (a5 + t * a6))))));
}
__device__ __forceinline__ double esati(double t)
{
  const double b0 = 6.109177956, b1 = 5.034698970e-01, b2 = 1.886013408e-02, b3 = 4.176223716e-04, b4 = 5.824720280e-06,
               b5 = 4.838803174e-08, b6 = 1.838826904e-10;
  return 100.0 * (b0 + t * (b1 + t * (b2 + t * (b3 + t * (b4 + t * (b5 + t * b6))))));
}

struct ForcingWeights {
  double wt1[8], wt2[8];  // TBOT, PBOT, QBOT|RH, FLDS, FSDS, PREC, WIND, ZBOT (the last three and FSDS unused)
  int qbot_is_rh;
};

// where a column reads its two records of each raw stream (TBOT PBOT QBOT FLDS FSDS PREC WIND): record t_idx at l0[k] + c,
// t_idx + 1 at l1[k] + c - the levels of atm_* for elmk_get_forcing, two slots of the forcing series for elmk_run
struct ForcingSrc {
  dfield l0[RUN_NFORC], l1[RUN_NFORC];
  __device__ __forceinline__ double get(int k, int lev, int64_t c) const { return lev ? (double)l1[k][c] : (double)l0[k][c]; }
};
#define SV(k, lev) src.l##lev[k][c]
#define FV(k, lev) src.get(k, lev, c)

// ---- downscaling to the column's elevation (include/elmk.h "downscaling"; ELM's downscale_forcings) -------------------------------
// tg, pg, qg, Lg: tbot, pbot, qbot, lwrad as get_forcing computes them at the forcing's surface height hf; the values at the column's
// elevation hc, in this operation order, without contraction (elmkernels_amd/downscale.py restates it on the host)
constexpr double DS_ZBOT = 30.0;  // ProcessZBOT's forc_hgt
struct DsCol {
  double tc, thc, pc, qc, lc;
};
__device__ __forceinline__ DsCol downscale_col(double tg, double pg, double qg, double lg, double hc, double hf, const DsParams& P)
{
  DsCol o;
  const double dz = hc - hf;
  o.tc = tg - P.lapse * dz;
  const double hbot = RAIR * 0.5 * (tg + o.tc) / GRAV;
  o.pc = pg * elmk_exp(-dz / hbot);
  o.thc = tg + (o.tc - tg) * elmk_exp((DS_ZBOT / hbot) * (RAIR / CPAIR));  // thg = tg (ProcessTBOT: forc_thbot = tbot)
  double es, esdT, qs_g, qs_c, qsdT;
  qsat(tg, pg, es, esdT, qs_g, qsdT);
  qsat(o.tc, o.pc, es, esdT, qs_c, qsdT);
  o.qc = qg * (qs_c / qs_g);
  o.lc = dmax(dmin(lg - P.lapse_lw * dz, lg * (1.0 + P.lw_limit)), lg * (1.0 - P.lw_limit));
  return o;
}

// one column: the body of k_get_forcing and of its run-mode variants; Src::get(k, lev, c) is record t_idx + lev of stream k at
// column c (ForcingSrc: per-column records; GridForcingSrc: cell records remapped through the forcing grid).  CZ: shortwave COSZEN
// mode, czf[c] the mean cos(zenith) of the column over the forcing record's interval.  DS: downscaling TOPO mode (*ds): tbot, thbot,
// pbot, qbot and lwrad at the column's elevation, rain and snow split by the downscaled temperature, Lg to ds->lg while groups are set.
template <bool CZ, class Src, bool DS = false>
__device__ __forceinline__ void get_forcing_col(const DevState* __restrict__ S, int64_t c, const ForcingWeights& W, const Src& src,
                                                const double* __restrict__ czf = nullptr, const DsParams* ds = nullptr)
{
  const int64_t ld = S->ld;
  // ProcessTBOT :38-42
  const double tbot = dmin(interp_forcing(W.wt1[0], W.wt2[0], FV(0, 0), FV(0, 1)), 323.0);
  if constexpr (!DS) {
    S->forc_tbot[c] = tbot;
    S->forc_thbot[c] = tbot;
  }
  // ProcessPBOT :55-58
  const double pbot = dmax(interp_forcing(W.wt1[1], W.wt2[1], FV(1, 0), FV(1, 1)), 4.0e4);
  if constexpr (!DS) S->forc_pbot[c] = pbot;
  // ProcessQBOT :73-81
  double qbot = dmax(interp_forcing(W.wt1[2], W.wt2[2], FV(2, 0), FV(2, 1)), 1.0e-9);
  if (W.qbot_is_rh) {
    const double e = (tbot > TFRZ) ? esatw(tdc(tbot)) : esati(tdc(tbot));
    const double qsat = 0.622 * e / (pbot - 0.378 * e);
    qbot *= qsat / 100.0;
  }
  if constexpr (!DS) S->forc_qbot[c] = qbot;
  // ProcessFLDS :97-107
  const double flds = interp_forcing(W.wt1[3], W.wt2[3], FV(3, 0), FV(3, 1));
  double lwrad = flds;
  if (flds <= 50.0 || flds >= 600.0) {
    const double e = pbot * qbot / (0.622 + 0.378 * qbot);
    const double ea = 0.70 + 5.95e-5 * 0.01 * e * elmk_exp(1500.0 / tbot);
    lwrad = ea * STEBOL * elmk_pow(tbot, 4.0);
  }
  double tprec = tbot;  // the temperature that splits precipitation
  if constexpr (DS) {
    const DsCol d = downscale_col(tbot, pbot, qbot, lwrad, ds->hc[c], ds->hf[c], *ds);
    S->forc_tbot[c] = d.tc;
    S->forc_thbot[c] = d.thc;
    S->forc_pbot[c] = d.pc;
    S->forc_qbot[c] = d.qc;
    S->forc_lwrad[c] = d.lc;
    if (ds->lg) ds->lg[c] = lwrad;
    tprec = d.tc;
  } else {
    S->forc_lwrad[c] = lwrad;
  }
  // ProcessFSDS :122-142 (record t_idx only); pow(x, 2.0) is x * x in the reference's optimised builds (elmk_math.h).  COSZEN:
  // the record (an interval mean) weighted by ELM's fac = (cosz > 0.001) ? min(cosz / avg_forc_cosz, 10) : 0 (:126-130)
  {
    double swndr;
    if constexpr (CZ) {
      const double cz = S->coszen[c];
      const double fac = (cz > 0.001) ? dmin(cz / czf[c], 10.0) : 0.0;
      swndr = dmax(FV(4, 0) * fac * 0.5, 0.0);
    } else {
      swndr = dmax(FV(4, 0) * S->coszen[c] * 0.5, 0.0);
    }
    const double swndf = swndr, swvdr = swndr, swvdf = swndr;
    const double ratio_rvrf_vis =
        dmin(0.99, dmax(0.17639 + 0.00380 * swvdr - 9.0039e-06 * elmk_sq(swvdr) + 8.1351e-09 * elmk_pow(swvdr, 3.0), 0.01));
    const double ratio_rvrf_nir =
        dmin(0.99, dmax(0.29548 + 0.00504 * swndr - 1.4957e-05 * elmk_sq(swndr) + 1.4881e-08 * elmk_pow(swndr, 3.0), 0.01));
    LV(forc_solad, 0) = ratio_rvrf_vis * swvdr;
    LV(forc_solad, 1) = ratio_rvrf_nir * swndr;
    LV(forc_solai, 0) = (1.0 - ratio_rvrf_vis) * swvdf;
    LV(forc_solai, 1) = (1.0 - ratio_rvrf_nir) * swndf;
  }
  // ProcessPREC :157-163 (record t_idx only)
  {
    const double frac1 = (tprec - TFRZ) * 0.5;
    const double frac2 = dmin(1.0, dmax(0.0, frac1));
    const double prec = dmax(FV(5, 0), 0.0);
    S->forc_rain[c] = frac2 * prec;
    S->forc_snow[c] = (1.0 - frac2) * prec;
  }
  // ProcessWIND :177-181
  S->forc_u[c] = interp_forcing(W.wt1[6], W.wt2[6], FV(6, 0), FV(6, 1));
  S->forc_v[c] = 0.0;
  // ProcessZBOT :195-203 (hardwired 30 m)
  S->forc_hgt[c] = 30.0;
  S->forc_hgt_u_patch[c] = 30.0;
  S->forc_hgt_t_patch[c] = 30.0;
  S->forc_hgt_q_patch[c] = 30.0;
}

// ---- forcing on a coarser grid (elmk_set_forcing_grid) -------------------------------------------------------------------------
// The map is ELL: NPTS rows idx[k][column] (int32) and w[k][column] (fp64), SoA with the state's level stride; idx = -1 is padding
// (every row k >= 1 may hold it, row 0 never does - elmk_api.cpp checks both on the host, so every gather is inside the cell
// record).  The value of column c is defined by this operation order (include/elmk.h), which regrid.apply_map restates on the host:
//   v = w[0] * a[idx[0]];  then for k = 1 .. NPTS-1: if idx[k] >= 0: v = v + w[k] * a[idx[k]]
// Padding is skipped, not multiplied by zero: -0.0 stays -0.0 and a non-finite cell behind a padding slot is never read.
// NPTS is wave-uniform (the map's width, rounded up to 1, 2, 4 or 8 with padding rows), so the loop is unrolled per width.
#ifndef ELMK_GRID_MAP_NT
// 1: nontemporal hint on the map loads.  Not taken: in an interleaved A/B at 1 M columns (profiles/r08_forcing_grid_cost.jsonl, the
// rows with "ab_lib") the hint made 6 of 8 grid configurations 1-4 % slower per step and 2 (nearest, ncols / 150 cells) 4-5 % faster.
#define ELMK_GRID_MAP_NT 0
#endif
template <typename T> __device__ __forceinline__ T map_load(gptr<const T> p)
{
  if (ELMK_GRID_MAP_NT) return __builtin_nontemporal_load(p);
  return *p;
}

template <int NPTS, class A>
__device__ __forceinline__ double remap_cells(const int32_t (&idx)[NPTS], const double (&w)[NPTS], const A& a)
{
  double v = w[0] * (double)a[idx[0]];
#pragma unroll
  for (int k = 1; k < NPTS; k++)
    if (idx[k] >= 0) v = v + w[k] * (double)a[idx[k]];
  return v;
}

// the map row of column c, loaded once (coalesced) and reused by every stream and record that column reads
template <int NPTS>
__device__ __forceinline__ void load_map_row(gptr<const int32_t> midx, gptr<const double> mw, int64_t ld, int64_t c, int32_t (&idx)[NPTS],
                                             double (&w)[NPTS])
{
#pragma unroll
  for (int k = 0; k < NPTS; k++) {
    idx[k] = map_load(midx + (int64_t)k * ld + c);
    w[k] = map_load(mw + (int64_t)k * ld + c);
  }
}

// the source of get_forcing_col in grid mode: record t_idx + lev of stream k is the cell record l0[k] / l1[k] remapped to column c
template <int NPTS> struct GridForcingSrc {
  dfield l0[RUN_NFORC], l1[RUN_NFORC];
  int32_t idx[NPTS];
  double w[NPTS];
  __device__ __forceinline__ double get(int k, int lev, int64_t) const { return remap_cells<NPTS>(idx, w, lev ? l1[k] : l0[k]); }
};

// the two months a column reads of mlai, msai, mhtop, mhbot (in this order): month start_idx at l0[k] + c, start_idx + 1 at
// l1[k] + c - the levels of the fields for elmk_phenology, two months of the phenology series for elmk_run
struct PhenologySrc {
  dfield l0[RUN_NPHEN], l1[RUN_NPHEN];
};

// phenology_physics_impl.hh:22-69, one column: the body of k_phenology and of its run-mode variant
__device__ __forceinline__ void phenology_col(const DevState* __restrict__ S, int64_t c, double wt1, double wt2, const PhenologySrc& src)
{
  constexpr int noveg = 0, nbrdlf_dcd_brl_shrub = 11;  // elm_constants.h:56,67
  const int vtype = S->vtype[c];
  double tlai = 0.0, tsai = 0.0, htop = 0.0, hbot = 0.0;
  if (vtype != noveg) {
    tlai = wt1 * SV(0, 0) + wt2 * SV(0, 1);
    tsai = wt1 * SV(1, 0) + wt2 * SV(1, 1);
    htop = wt1 * SV(2, 0) + wt2 * SV(2, 1);
    hbot = wt1 * SV(3, 0) + wt2 * SV(3, 1);
  }
  S->tlai[c] = tlai;
  S->tsai[c] = tsai;
  S->htop[c] = htop;
  S->hbot[c] = hbot;
  const double snow_depth = S->snow_depth[c], frac_sno = S->frac_sno[c];
  double fb;
  if (vtype > noveg && vtype <= nbrdlf_dcd_brl_shrub) {
    const double ol = dmin(dmax(snow_depth - hbot, 0.0), htop - hbot);
    fb = 1.0 - ol / dmax(1.e-06, htop - hbot);
  } else {
    fb = 1.0 - dmax(dmin(snow_depth, 0.2), 0.0) / 0.2;  // 0.2 m buries grasses
  }
  double elai = dmax(tlai * (1.0 - frac_sno) + tlai * fb * frac_sno, 0.0);
  double esai = dmax(tsai * (1.0 - frac_sno) + tsai * fb * frac_sno, 0.0);
  if (elai < 0.05) elai = 0.0;
  if (esai < 0.05) esai = 0.0;
  S->elai[c] = elai;
  S->esai[c] = esai;
  S->frac_veg_nosno_alb[c] = ((elai + esai) >= 0.05) ? 1 : 0;
}

template <bool CZ>
__device__ __forceinline__ void get_forcing_levels(const DevState* __restrict__ S, const ForcingWeights& W, const double* __restrict__ czf)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const ForcingSrc src{{S->atm_tbot, S->atm_pbot, S->atm_qbot, S->atm_flds, S->atm_fsds, S->atm_prec, S->atm_wind},
                       {S->atm_tbot + ld, S->atm_pbot + ld, S->atm_qbot + ld, S->atm_flds + ld, S->atm_fsds + ld, S->atm_prec + ld,
                        S->atm_wind + ld}};
  get_forcing_col<CZ>(S, c, W, src, czf);
}

__global__ __launch_bounds__(256) void k_get_forcing(const DevState* __restrict__ S, const ForcingWeights W)
{
  get_forcing_levels<false>(S, W, nullptr);
}

__global__ __launch_bounds__(256) void k_get_forcing_cz(const DevState* __restrict__ S, const ForcingWeights W, const double* __restrict__ czf)
{
  get_forcing_levels<true>(S, W, czf);
}

// TOPO mode (elmk_set_downscaling): the downscaling variants of the kernels around them, COSZEN through CZ (czf null without it).
// New kernels, so each shares one template; the OFF kernels keep their own bodies (see the note above k_get_forcing_run_cz).
template <bool CZ>
__global__ __launch_bounds__(256) void k_get_forcing_ds(const DevState* __restrict__ S, const ForcingWeights W, const double* __restrict__ czf,
                                                        const DsParams P)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const ForcingSrc src{{S->atm_tbot, S->atm_pbot, S->atm_qbot, S->atm_flds, S->atm_fsds, S->atm_prec, S->atm_wind},
                       {S->atm_tbot + ld, S->atm_pbot + ld, S->atm_qbot + ld, S->atm_flds + ld, S->atm_fsds + ld, S->atm_prec + ld,
                        S->atm_wind + ld}};
  get_forcing_col<CZ, ForcingSrc, true>(S, c, W, src, czf, &P);
}

__global__ __launch_bounds__(256) void k_phenology(const DevState* __restrict__ S, double wt1, double wt2)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const PhenologySrc src{{S->mlai, S->msai, S->mhtop, S->mhbot}, {S->mlai + ld, S->msai + ld, S->mhtop + ld, S->mhbot + ld}};
  phenology_col(S, c, wt1, wt2, src);
}

// elmk_run: the weights and the records of the step's row of the step table, from the series (elmk_api.cpp: elmk_run_reserve)
__device__ __forceinline__ void run_weights(const RunRow* __restrict__ r, int qbot_is_rh, ForcingWeights& W)
{
#pragma unroll
  for (int i = 0; i < 8; i++) {
    W.wt1[i] = r->forc_wt1[i];
    W.wt2[i] = r->forc_wt2[i];
  }
  W.qbot_is_rh = qbot_is_rh;
}

__global__ __launch_bounds__(256) void k_get_forcing_run(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                         const int32_t* __restrict__ cursor, const dfield forc, int slots, int qbot_is_rh)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  ForcingSrc src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ld;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ld;
  }
  get_forcing_col<false>(S, c, W, src);
}

// (the COSZEN kernels repeat the bodies of the REFERENCE ones instead of sharing them through a helper: inlined through a helper, the
// REFERENCE kernels' code changed, if only in the operand order of an address add)
__global__ __launch_bounds__(256) void k_get_forcing_run_cz(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                            const int32_t* __restrict__ cursor, const dfield forc, int slots, int qbot_is_rh,
                                                            const double* __restrict__ czf)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  ForcingSrc src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ld;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ld;
  }
  get_forcing_col<true>(S, c, W, src, czf);
}

template <bool CZ>
__global__ __launch_bounds__(256) void k_get_forcing_run_ds(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                            const int32_t* __restrict__ cursor, const dfield forc, int slots, int qbot_is_rh,
                                                            const double* __restrict__ czf, const DsParams P)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  ForcingSrc src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ld;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ld;
  }
  get_forcing_col<CZ, ForcingSrc, true>(S, c, W, src, czf, &P);
}

// elmk_run with a forcing grid: the series hold cell records [RUN_NFORC][slots][ncells]; the body is k_get_forcing_run's, fed the
// remapped records (FSDS and PREC read record t_idx only, as there)
template <int NPTS>
__global__ __launch_bounds__(256) void k_get_forcing_run_grid(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                              const int32_t* __restrict__ cursor, const dfield forc, int slots,
                                                              int64_t ncells, gptr<const int32_t> midx, gptr<const double> mw, int qbot_is_rh)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  GridForcingSrc<NPTS> src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ncells;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ncells;
  }
  load_map_row<NPTS>(midx, mw, ld, c, src.idx, src.w);
  get_forcing_col<false>(S, c, W, src);
}

template <int NPTS>
__global__ __launch_bounds__(256) void k_get_forcing_run_grid_cz(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ cursor, const dfield forc, int slots,
                                                                 int64_t ncells, gptr<const int32_t> midx, gptr<const double> mw,
                                                                 int qbot_is_rh, const double* __restrict__ czf)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  GridForcingSrc<NPTS> src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ncells;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ncells;
  }
  load_map_row<NPTS>(midx, mw, ld, c, src.idx, src.w);
  get_forcing_col<true>(S, c, W, src, czf);
}

template <int NPTS, bool CZ>
__global__ __launch_bounds__(256) void k_get_forcing_run_grid_ds(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                                 const int32_t* __restrict__ cursor, const dfield forc, int slots,
                                                                 int64_t ncells, gptr<const int32_t> midx, gptr<const double> mw,
                                                                 int qbot_is_rh, const double* __restrict__ czf, const DsParams P)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  ForcingWeights W;
  run_weights(r, qbot_is_rh, W);
  const int64_t slot = r->forc_slot;
  GridForcingSrc<NPTS> src;
#pragma unroll
  for (int k = 0; k < RUN_NFORC; k++) {
    src.l0[k] = forc + ((int64_t)k * slots + slot) * ncells;
    src.l1[k] = forc + ((int64_t)k * slots + slot + 1) * ncells;
  }
  load_map_row<NPTS>(midx, mw, ld, c, src.idx, src.w);
  get_forcing_col<CZ, GridForcingSrc<NPTS>, true>(S, c, W, src, czf, &P);
}

// elmk_upload_gridded: one level of an fp64 field from fp64 cell values (stored at state precision: fp32 in libelmk_f32.so)
template <int NPTS>
__global__ __launch_bounds__(256) void k_remap_field(dfield dst, gptr<const double> cells, int64_t n, int64_t ld, gptr<const int32_t> midx,
                                                     gptr<const double> mw)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  int32_t idx[NPTS];
  double w[NPTS];
  load_map_row<NPTS>(midx, mw, ld, c, idx, w);
  dst[c] = remap_cells<NPTS>(idx, w, cells);
}

// elmk_set_forcing_elevation_gridded: k_remap_field into an fp64 row in every build (the elevations stay fp64 in libelmk_f32.so)
template <int NPTS>
__global__ __launch_bounds__(256) void k_remap_field_f64(gptr<double> dst, gptr<const double> cells, int64_t n, int64_t ld,
                                                         gptr<const int32_t> midx, gptr<const double> mw)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  int32_t idx[NPTS];
  double w[NPTS];
  load_map_row<NPTS>(midx, mw, ld, c, idx, w);
  dst[c] = remap_cells<NPTS>(idx, w, cells);
}

__global__ __launch_bounds__(256) void k_phenology_run(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                       const int32_t* __restrict__ cursor, const dfield phen)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ld = S->ld;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  const int64_t m1 = r->month1, m2 = r->month2;
  PhenologySrc src;
#pragma unroll
  for (int k = 0; k < RUN_NPHEN; k++) {
    src.l0[k] = phen + ((int64_t)k * RUN_NMONTH + m1) * ld;
    src.l1[k] = phen + ((int64_t)k * RUN_NMONTH + m2) * ld;
  }
  phenology_col(S, c, r->month_wt1, r->month_wt2, src);
}

void launch_get_forcing(const DevState* S, int64_t n, const double* wt1, const double* wt2, int qbot_is_rh, hipStream_t st,
                        const double* czf, const DsParams* ds)
{
  if (n <= 0) return;
  ForcingWeights W;
  for (int i = 0; i < 8; i++) {
    W.wt1[i] = wt1[i];
    W.wt2[i] = wt2[i];
  }
  W.qbot_is_rh = qbot_is_rh;
  if (ds) {
    if (czf)
      hipLaunchKernelGGL(k_get_forcing_ds<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, W, czf, *ds);
    else
      hipLaunchKernelGGL(k_get_forcing_ds<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, W, czf, *ds);
    return;
  }
  if (czf)
    hipLaunchKernelGGL(k_get_forcing_cz, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, W, czf);
  else
    hipLaunchKernelGGL(k_get_forcing, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, W);
}

void launch_phenology(const DevState* S, int64_t n, double wt1, double wt2, hipStream_t st)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_phenology, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, wt1, wt2);
}

void launch_get_forcing_run(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, const void* forc, int slots,
                            int qbot_is_rh, hipStream_t st, const double* czf, const DsParams* ds)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const dfield f = field_of<ELMK_F64>::from(const_cast<void*>(forc));
  if (ds) {
    if (czf)
      hipLaunchKernelGGL(k_get_forcing_run_ds<true>, grid, block, 0, st, S, rows, cursor, f, slots, qbot_is_rh, czf, *ds);
    else
      hipLaunchKernelGGL(k_get_forcing_run_ds<false>, grid, block, 0, st, S, rows, cursor, f, slots, qbot_is_rh, czf, *ds);
    return;
  }
  if (czf)
    hipLaunchKernelGGL(k_get_forcing_run_cz, grid, block, 0, st, S, rows, cursor, f, slots, qbot_is_rh, czf);
  else
    hipLaunchKernelGGL(k_get_forcing_run, grid, block, 0, st, S, rows, cursor, f, slots, qbot_is_rh);
}

void launch_get_forcing_run_grid(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, const void* forc, int slots,
                                 int64_t ncells, int npts, const int32_t* idx, const double* w, int qbot_is_rh, hipStream_t st,
                                 const double* czf, const DsParams* ds)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const dfield f = field_of<ELMK_F64>::from(const_cast<void*>(forc));
  const gptr<const int32_t> mi = (gptr<const int32_t>)idx;
  const gptr<const double> mw = (gptr<const double>)w;
  if (ds) {
#define ELMK_DS_GRID(N, CZ) hipLaunchKernelGGL((k_get_forcing_run_grid_ds<N, CZ>), grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh, czf, *ds)
    switch (npts) {
      case 1: if (czf) ELMK_DS_GRID(1, true); else ELMK_DS_GRID(1, false); break;
      case 2: if (czf) ELMK_DS_GRID(2, true); else ELMK_DS_GRID(2, false); break;
      case 4: if (czf) ELMK_DS_GRID(4, true); else ELMK_DS_GRID(4, false); break;
      default: if (czf) ELMK_DS_GRID(8, true); else ELMK_DS_GRID(8, false); break;
    }
#undef ELMK_DS_GRID
    return;
  }
  if (czf) {
    switch (npts) {
      case 1: hipLaunchKernelGGL(k_get_forcing_run_grid_cz<1>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh, czf); break;
      case 2: hipLaunchKernelGGL(k_get_forcing_run_grid_cz<2>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh, czf); break;
      case 4: hipLaunchKernelGGL(k_get_forcing_run_grid_cz<4>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh, czf); break;
      default: hipLaunchKernelGGL(k_get_forcing_run_grid_cz<8>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh, czf); break;
    }
    return;
  }
  switch (npts) {
    case 1: hipLaunchKernelGGL(k_get_forcing_run_grid<1>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh); break;
    case 2: hipLaunchKernelGGL(k_get_forcing_run_grid<2>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh); break;
    case 4: hipLaunchKernelGGL(k_get_forcing_run_grid<4>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh); break;
    default: hipLaunchKernelGGL(k_get_forcing_run_grid<8>, grid, block, 0, st, S, rows, cursor, f, slots, ncells, mi, mw, qbot_is_rh); break;
  }
}

void launch_remap_field(void* dst, const double* cells, int64_t n, int64_t ld, int npts, const int32_t* idx, const double* w, hipStream_t st)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const dfield d = field_of<ELMK_F64>::from(dst);
  const gptr<const double> a = (gptr<const double>)cells;
  const gptr<const int32_t> mi = (gptr<const int32_t>)idx;
  const gptr<const double> mw = (gptr<const double>)w;
  switch (npts) {
    case 1: hipLaunchKernelGGL(k_remap_field<1>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    case 2: hipLaunchKernelGGL(k_remap_field<2>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    case 4: hipLaunchKernelGGL(k_remap_field<4>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    default: hipLaunchKernelGGL(k_remap_field<8>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
  }
}

void launch_remap_field_f64(double* dst, const double* cells, int64_t n, int64_t ld, int npts, const int32_t* idx, const double* w,
                            hipStream_t st)
{
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  const gptr<double> d = (gptr<double>)dst;
  const gptr<const double> a = (gptr<const double>)cells;
  const gptr<const int32_t> mi = (gptr<const int32_t>)idx;
  const gptr<const double> mw = (gptr<const double>)w;
  switch (npts) {
    case 1: hipLaunchKernelGGL(k_remap_field_f64<1>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    case 2: hipLaunchKernelGGL(k_remap_field_f64<2>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    case 4: hipLaunchKernelGGL(k_remap_field_f64<4>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
    default: hipLaunchKernelGGL(k_remap_field_f64<8>, grid, block, 0, st, d, a, n, ld, mi, mw); break;
  }
}

void launch_phenology_run(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, const void* phen, hipStream_t st)
{
  if (n <= 0) return;
  hipLaunchKernelGGL(k_phenology_run, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, rows, cursor,
                     field_of<ELMK_F64>::from(const_cast<void*>(phen)));
}

}  // namespace elmk
