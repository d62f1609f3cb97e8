// demo_site.h - the synthetic site of the examples that drive single stages through the C ABI (include/elmk.h): uniform loam columns
// on ELM's soil grid, the soil hydrology switched on, and, for the river demos, one output cell per column with the routing on it.
// A demo says what differs (how wet, how conductive, which cell drains where) and goes on to its own subject.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "elmk.h"

namespace demo {

inline void chk(elmk_ctx* ctx, int rc, const char* what)
{
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + elmk_last_error(ctx));
}
inline int fid(const char* name)
{
  const int f = elmk_field_id(name);
  if (f < 0) throw std::runtime_error(std::string("no field ") + name);
  return f;
}
// one value per level for every column, [column][level]
inline void put(elmk_ctx* ctx, const char* name, int64_t n, const std::vector<double>& levels)
{
  std::vector<double> a((size_t)n * levels.size());
  for (int64_t c = 0; c < n; c++)
    for (size_t l = 0; l < levels.size(); l++) a[(size_t)c * levels.size() + l] = levels[l];
  chk(ctx, elmk_upload(ctx, fid(name), a.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), name);
}

// ELM's soil grid: 5 snow levels (unused here, left zero), 15 ground layers; zi[21] interfaces, dz[20] thicknesses, z[20] nodes
inline void soil_grid(std::vector<double>& zi, std::vector<double>& dz, std::vector<double>& z)
{
  zi.assign(21, 0.0), dz.assign(20, 0.0), z.assign(20, 0.0);
  for (int j = 0; j < 15; j++) z[5 + j] = 0.025 * (std::exp(0.5 * (j + 0.5)) - 1.0);
  for (int j = 0; j < 15; j++) zi[6 + j] = j < 14 ? 0.5 * (z[5 + j] + z[6 + j]) : z[19] + 0.5 * (z[19] - z[18]);
  for (int j = 0; j < 15; j++) dz[5 + j] = zi[6 + j] - zi[5 + j];
}

constexpr double WATSAT = 0.45, SUCSAT = 200.0, BSW = 5.0;  // the loam

// n uniform loam columns without ice, every ground layer filled to the fraction `sat` of its pore space
inline void loam_columns(elmk_ctx* ctx, int64_t n, double sat)
{
  std::vector<double> zi, dz, z, liq(20, 0.0);
  soil_grid(zi, dz, z);
  for (int j = 0; j < 15; j++) liq[5 + j] = sat * WATSAT * dz[5 + j] * 1000.0;
  put(ctx, "zisoi", n, zi);
  put(ctx, "dz", n, dz);
  put(ctx, "zsoi", n, z);
  put(ctx, "h2osoi_liq", n, liq);
  put(ctx, "h2osoi_ice", n, std::vector<double>(20, 0.0));
  put(ctx, "watsat", n, std::vector<double>(15, WATSAT));
  put(ctx, "sucsat", n, std::vector<double>(15, SUCSAT));
  put(ctx, "bsw", n, std::vector<double>(15, BSW));
}

// the soil hydrology stage with uniform parameters: hksat mm/s in every layer, wtfact, thresh 5, k_wet, rsub
inline void hydrology_on(elmk_ctx* ctx, int64_t n, double hksat, double wtfact = 0.4, double k_wet = 0.035, double rsub = 0.35)
{
  chk(ctx, elmk_soil_hydrology_enable(ctx), "elmk_soil_hydrology_enable");
  const std::vector<double> k((size_t)ELMK_HYD_NLAYER * n, hksat), f(n, wtfact), thresh(n, 5.0), kw(n, k_wet), r(n, rsub);
  chk(ctx, elmk_soil_hydrology_set_params(ctx, k.data(), f.data(), thresh.data(), kw.data(), r.data()), "elmk_soil_hydrology_set_params");
}
// its start values: the water table zwt0 m deep in every column, 4000 mm in the aquifer
inline void hydrology_start(elmk_ctx* ctx, int64_t n, double zwt0)
{
  const std::vector<double> zwt(n, zwt0), wa(n, 4000.0);
  chk(ctx, elmk_soil_hydrology_init(ctx, zwt.data(), wa.data()), "elmk_soil_hydrology_init");
}

// a chain of n cells: cell c drains into c + 1, the last is the outlet
inline std::vector<int32_t> chain(int64_t n)
{
  std::vector<int32_t> down((size_t)n);
  for (int64_t c = 0; c < n; c++) down[c] = c + 1 < n ? (int32_t)(c + 1) : -1;
  return down;
}

// the output grid of a river demo, one column per cell with weight one, and the routing on it: cells of 100 km2, 20 km from their
// downstream cell down[c] (-1: an outlet), effective velocity 0.35 m/s, nsub substeps
inline void river_cells(elmk_ctx* ctx, const std::vector<int32_t>& down, int nsub)
{
  const int64_t n = (int64_t)down.size();
  std::vector<int64_t> ptr(n + 1);
  std::vector<int32_t> col(n);
  const std::vector<double> w(n, 1.0), ddist(n, 2.0e4), area(n, 1.0e8);
  for (int64_t c = 0; c <= n; c++) ptr[c] = c;
  for (int64_t c = 0; c < n; c++) col[c] = (int32_t)c;
  chk(ctx, elmk_set_output_grid(ctx, n, ptr.data(), col.data(), w.data(), 0.0), "elmk_set_output_grid");
  chk(ctx, elmk_routing_enable(ctx, n, down.data(), ddist.data(), area.data(), 0.35, nsub), "elmk_routing_enable");
}

// the kinematic-wave scheme with the same eleven values in every cell: params[ELMK_KW_NPARAM][n]
inline void kinematic_on(elmk_ctx* ctx, int64_t n, const double value[ELMK_KW_NPARAM])
{
  std::vector<double> params((size_t)ELMK_KW_NPARAM * n);
  for (int k = 0; k < ELMK_KW_NPARAM; k++)
    for (int64_t c = 0; c < n; c++) params[(size_t)k * n + c] = value[k];
  chk(ctx, elmk_routing_kinematic_enable(ctx, params.data()), "elmk_routing_kinematic_enable");
}

}  // namespace demo
