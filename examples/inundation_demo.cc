// inundation_demo.cc - the kinematic-wave scheme's main channel with and without banks (elmk.h "floodplain inundation"), through the C
// ABI: the storm of kinematic_routing_demo.cc on its chain of eight cells, one uniform loam column per cell.  Two contexts step the
// same columns through six hours of heavy rain and eighteen hours without and route the runoff through hillslope, tributaries and main
// channel; in the second the channel has banks of 0.25 m and a floodplain that rises 0.2 m per tenth of the cell, so what exceeds the
// channel spreads out, stands still and comes back as the river falls.  Prints the outlet's discharge under both per step and the
// outlet cell's flooded fraction, then each hydrograph's peak and its step, every cell's largest flooded fraction, and what the
// floodplains still hold.  In a model run elmk_run with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING does all of
// it on the device.  The columns, the cells and the kinematic scheme come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/inundation_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o inundation_demo
//   ./inundation_demo
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 8;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4;

static elmk_ctx* make(bool banks)
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.7);
  hydrology_on(ctx, N, 2.0e-3);
  hydrology_start(ctx, N, 1.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, chain(N), NSUB);
  // a hillslope of 5 % with rough ground, 100 km of 10 m tributaries, a 20 km main channel 100 m wide
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  if (banks) {
    // rdepth[N] and eprof[ELMK_FP_NPROF][N]: banks of 0.25 m; the k-th tenth of the floodplain is wet at 0.2 k metres above them
    std::vector<double> rdepth(N, 0.25), eprof((size_t)ELMK_FP_NPROF * N);
    for (int k = 0; k < ELMK_FP_NPROF; k++)
      for (int64_t c = 0; c < N; c++) eprof[(size_t)k * N + c] = 0.2 * k;
    chk(ctx, elmk_routing_inundation_enable(ctx, rdepth.data(), eprof.data()), "elmk_routing_inundation_enable");
  }
  return ctx;
}

int main()
{
  elmk_ctx* both[2] = {nullptr, nullptr};
  try {
    const double dt = 1800.0, storm = 4.0e-3 /* mm/s: 14.4 mm/h */;
    const int nsteps = 48, storm_steps = 12;
    both[0] = make(false);
    both[1] = make(true);
    std::printf("a storm of %.1f mm in %d steps of %.0f s on a chain of %lld cells of 100 km2; discharge at the outlet, m3/s\n",
                storm * dt * storm_steps, storm_steps, dt, (long long)N);
    std::printf("%4s %10s %14s %14s %10s\n", "step", "rain mm/s", "no banks", "banks", "flooded");
    double peak[2] = {0.0, 0.0}, volume[2] = {0.0, 0.0};
    int peak_step[2] = {-1, -1};
    std::vector<double> frac(N), most(N, 0.0);
    for (int s = 0; s < nsteps; s++) {
      const double rain = s < storm_steps ? storm : 0.0;
      double q[2];
      for (int k = 0; k < 2; k++) {
        elmk_ctx* ctx = both[k];
        put(ctx, "qflx_top_soil", N, {rain});
        put(ctx, "forc_rain", N, {rain});
        chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
        chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
        chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
        chk(ctx, elmk_water_balance(ctx, dt, nullptr, nullptr, nullptr), "elmk_water_balance");
        chk(ctx, elmk_routing(ctx, dt), "elmk_routing");  // the flood form while the extension is on
        chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_QOUT, &q[k], N - 1, 1), "elmk_routing_read");
        volume[k] += q[k] * dt;
        if (q[k] > peak[k]) {
          peak[k] = q[k];
          peak_step[k] = s;
        }
      }
      chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_FLOOD_FRAC, frac.data(), 0, N), "elmk_routing_read");
      for (int64_t c = 0; c < N; c++)
        if (frac[c] > most[c]) most[c] = frac[c];
      std::printf("%4d %10.1e %14.6e %14.6e %10.6f\n", s, rain, q[0], q[1], frac[N - 1]);
    }
    double sums[3], kw[2], wf[1];
    chk(both[1], elmk_routing_budget(both[1], sums), "elmk_routing_budget");
    chk(both[1], elmk_routing_kinematic_budget(both[1], kw), "elmk_routing_kinematic_budget");
    chk(both[1], elmk_routing_inundation_budget(both[1], wf), "elmk_routing_inundation_budget");
    std::printf("no banks: peak %.4e m3/s at step %d, %.4e m3 through the outlet\n", peak[0], peak_step[0], volume[0]);
    std::printf("banks:    peak %.4e m3/s at step %d, %.4e m3 through the outlet\n", peak[1], peak_step[1], volume[1]);
    std::printf("largest flooded fraction per cell:");
    for (int64_t c = 0; c < N; c++) std::printf(" %.6f", most[c]);
    std::printf("\nbanks: still held on the hillslopes %.4e m3, in the tributaries %.4e m3, in the main channels %.4e m3, on the floodplains %.4e m3\n",
                kw[0], kw[1], sums[0], wf[0]);
    const bool ok = peak[0] > 0.0 && peak[1] > 0.0 && peak[1] <= peak[0] && wf[0] >= 0.0;
    chk(both[1], elmk_routing_inundation_clear(both[1]), "elmk_routing_inundation_clear");  // (elmk_routing_clear would free it as well)
    for (int k = 0; k < 2; k++) {
      chk(both[k], elmk_routing_clear(both[k]), "elmk_routing_clear");
      chk(both[k], elmk_destroy(both[k]), "elmk_destroy");
    }
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "inundation_demo: %s\n", e.what());
    return 1;
  }
}
