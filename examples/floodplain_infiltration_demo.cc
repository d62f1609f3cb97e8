// floodplain_infiltration_demo.cc - floodplain water infiltrates the soil under it (elmk.h "floodplain infiltration"), through the C
// ABI: the storm of inundation_demo.cc on its chain of eight cells with banks, one uniform loam column per cell, dry at the start.  Two
// contexts step the same columns through six hours of heavy rain and eighteen hours without; in the second the extension is on, so
// the columns of the flooded cells wet from below the standing water (QFLX_H2OROF_DRAIN joins QFLX_INFL) while the routing takes the
// same water out of WF.  Prints per step the floodplains' water and the columns' soil water under both, what the land took, then the
// budget of land and river together: what the columns gained is what the floodplains lost.  In a model run elmk_run with
// ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING does all of it on the device.  The columns, the cells and the
// kinematic scheme come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/floodplain_infiltration_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o floodplain_infiltration_demo
//   ./floodplain_infiltration_demo
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 8;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4;

static elmk_ctx* make(bool infiltration)
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.4);  // dry soil: room for the flood's water
  hydrology_on(ctx, N, 2.0e-3);
  hydrology_start(ctx, N, 3.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, chain(N), NSUB);
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  std::vector<double> rdepth(N, 0.25), eprof((size_t)ELMK_FP_NPROF * N);
  for (int k = 0; k < ELMK_FP_NPROF; k++)
    for (int64_t c = 0; c < N; c++) eprof[(size_t)k * N + c] = 0.2 * k;
  chk(ctx, elmk_routing_inundation_enable(ctx, rdepth.data(), eprof.data()), "elmk_routing_inundation_enable");
  // after the hydrology, the water balance, the scheme and the inundation; every column of the output grid is in one cell
  if (infiltration) chk(ctx, elmk_floodplain_infiltration_enable(ctx), "elmk_floodplain_infiltration_enable");
  return ctx;
}

static double total(const std::vector<double>& a)
{
  double s = 0.0;
  for (double v : a) s += v;
  return s;
}

int main()
{
  elmk_ctx* both[2] = {nullptr, nullptr};
  try {
    const double dt = 1800.0, storm = 8.0e-3 /* mm/s: 28.8 mm/h, far above what the loam takes */, area = 1.0e8;
    const int nsteps = 48, storm_steps = 12;
    both[0] = make(false);
    both[1] = make(true);
    std::printf("a storm of %.1f mm in %d steps of %.0f s on a chain of %lld cells of 100 km2 with banks of 0.25 m\n", storm * dt * storm_steps,
                storm_steps, dt, (long long)N);
    std::printf("%4s %14s %14s %16s %16s %14s\n", "step", "WF plain m3", "WF coupled m3", "soil plain mm", "soil coupled mm", "land took m3");
    std::vector<double> wf(N), liq(N), qland(N), drain(N), frac(N);
    double took = 0.0, soil[2] = {0.0, 0.0}, flood[2] = {0.0, 0.0}, most = 0.0;
    for (int s = 0; s < nsteps; s++) {
      const double rain = s < storm_steps ? storm : 0.0;
      for (int k = 0; k < 2; k++) {
        elmk_ctx* ctx = both[k];
        put(ctx, "qflx_top_soil", N, {rain});
        put(ctx, "forc_rain", N, {rain});
        chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
        chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
        chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");                      // F1 - F3 while the extension is on
        chk(ctx, elmk_water_balance(ctx, dt, nullptr, nullptr, nullptr), "elmk_water_balance");  // F4
        chk(ctx, elmk_routing(ctx, dt), "elmk_routing");                                    // F5, with the same dt
        chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_WF, wf.data(), 0, N), "elmk_routing_read");
        chk(ctx, elmk_water_balance_read(ctx, ELMK_WB_TOTSOILLIQ, liq.data(), 0, N), "elmk_water_balance_read");
        flood[k] = total(wf);
        soil[k] = total(liq) / (double)N;
      }
      chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_QLAND, qland.data(), 0, N), "elmk_routing_read");
      chk(both[1], elmk_floodplain_infiltration_read(both[1], ELMK_FPI_QFLX_DRAIN, drain.data(), 0, N), "elmk_floodplain_infiltration_read");
      chk(both[1], elmk_floodplain_infiltration_read(both[1], ELMK_FPI_FRAC, frac.data(), 0, N), "elmk_floodplain_infiltration_read");
      for (int64_t c = 0; c < N; c++)
        if (frac[c] > most) most = frac[c];
      took += total(qland) * dt;
      std::printf("%4d %14.6e %14.6e %16.6f %16.6f %14.6e\n", s, flood[0], flood[1], soil[0], soil[1], total(qland) * dt);
    }
    double sums[1];
    chk(both[1], elmk_floodplain_infiltration_budget(both[1], sums), "elmk_floodplain_infiltration_budget");
    const double gained = (soil[1] - soil[0]) * (double)N * 0.001 * area;
    std::printf("the land took %.4e m3 from the floodplains; the coupled columns hold %.4e m3 more soil water than the plain ones\n", took, gained);
    std::printf("largest share of a cell under water: %.6f; sum of QLAND in the last step %.6e m3/s\n", most, sums[0]);
    const bool ok = took > 0.0 && soil[1] > soil[0] && most > 0.0 && sums[0] >= 0.0;
    chk(both[1], elmk_floodplain_infiltration_clear(both[1]), "elmk_floodplain_infiltration_clear");  // (elmk_routing_clear would free it as well)
    for (int k = 0; k < 2; k++) {
      chk(both[k], elmk_routing_clear(both[k]), "elmk_routing_clear");
      chk(both[k], elmk_destroy(both[k]), "elmk_destroy");
    }
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "floodplain_infiltration_demo: %s\n", e.what());
    return 1;
  }
}
