// reservoir_demo.cc - one dam on the kinematic-wave scheme's chain (elmk.h "reservoirs"), through the C ABI: eight cells, one uniform loam
// column per cell, and a year of twelve short "months" of eight half-hour steps each, wet in the first half and dry in the second.  Two
// contexts step the same columns and route the runoff through hillslope, tributaries and main channel; in the second a dam of 1e9 m3
// stands at the outlet of cell 4 with a target release of 150 m3/s in every month, BETA = 1 and an operational year that begins in month
// 0.  elmk_routing_reservoir_time tells the routing the month, and on a month's first step that it begins.  Prints the outlet's
// discharge with and without the dam and the reservoir's storage per step, then both hydrographs' range.  In a model run elmk_run with
// ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING does all of it on the device and takes the month from the step's date.
// The columns, the cells and the kinematic scheme come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/reservoir_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o reservoir_demo
//   ./reservoir_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 8;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4;

static const int64_t DAM = 4;
static const double CAP = 1.0e9;

static elmk_ctx* make(bool dam)
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
  if (dam) {
    // cap[N] (0 = no dam), target[12][N], beta[N], mstart[N]
    std::vector<double> cap(N, 0.0), target((size_t)12 * N, 0.0), beta(N, 0.0);
    std::vector<int32_t> mstart(N, 0);
    cap[DAM] = CAP;
    beta[DAM] = 1.0;
    for (int m = 0; m < 12; m++) target[(size_t)m * N + DAM] = 150.0;
    chk(ctx, elmk_routing_reservoir_enable(ctx, cap.data(), target.data(), beta.data(), mstart.data()), "elmk_routing_reservoir_enable");
    std::vector<double> res(N, 0.0);
    res[DAM] = 0.3 * CAP;
    chk(ctx, elmk_routing_reservoir_init(ctx, res.data(), nullptr), "elmk_routing_reservoir_init");
  }
  return ctx;
}

int main()
{
  elmk_ctx* both[2] = {nullptr, nullptr};
  try {
    const double dt = 1800.0;
    const int per_month = 8, nsteps = 12 * per_month;
    both[0] = make(false);
    both[1] = make(true);
    std::printf("twelve months of %d steps of %.0f s on a chain of %lld cells of 100 km2, a dam of %.1e m3 at cell %lld; discharge at the outlet, m3/s\n",
                per_month, dt, (long long)N, CAP, (long long)DAM);
    std::printf("%4s %5s %10s %14s %14s %14s\n", "step", "month", "rain mm/s", "no dam", "dam", "RES m3");
    double lo[2] = {1e300, 1e300}, hi[2] = {0.0, 0.0}, res = 0.0, res_lo = 1e300, res_hi = -1e300;
    for (int s = 0; s < nsteps; s++) {
      const int month = s / per_month;
      const double rain = 2.0e-3 * (1.0 + std::cos(2.0 * 3.14159265358979 * (month + 0.5) / 12.0)) * (s % per_month < 4 ? 1.0 : 0.25);
      double q[2];
      for (int k = 0; k < 2; k++) {
        elmk_ctx* ctx = both[k];
        put(ctx, "qflx_top_soil", N, {rain});
        put(ctx, "forc_rain", N, {rain});
        chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
        chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
        chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
        chk(ctx, elmk_water_balance(ctx, dt, nullptr, nullptr, nullptr), "elmk_water_balance");
        if (k == 1) chk(ctx, elmk_routing_reservoir_time(ctx, month, s % per_month == 0), "elmk_routing_reservoir_time");
        chk(ctx, elmk_routing(ctx, dt), "elmk_routing");  // the DAM form while the extension is on
        chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_QOUT, &q[k], N - 1, 1), "elmk_routing_read");
        if (s >= per_month) {  // (the first month fills the channels)
          if (q[k] < lo[k]) lo[k] = q[k];
          if (q[k] > hi[k]) hi[k] = q[k];
        }
      }
      chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_RES, &res, DAM, 1), "elmk_routing_read");
      if (res < res_lo) res_lo = res;
      if (res > res_hi) res_hi = res;
      std::printf("%4d %5d %10.2e %14.6e %14.6e %14.6e\n", s, month, rain, q[0], q[1], res);
    }
    double sums[2], krls = 0.0;
    chk(both[1], elmk_routing_reservoir_budget(both[1], sums), "elmk_routing_reservoir_budget");
    chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_KRLS, &krls, DAM, 1), "elmk_routing_read");
    std::printf("no dam: the outlet ranges over %.4e .. %.4e m3/s\n", lo[0], hi[0]);
    std::printf("dam:    the outlet ranges over %.4e .. %.4e m3/s; the reservoir over %.4e .. %.4e m3, now %.4e m3, KRLS %.6f\n", lo[1], hi[1],
                res_lo, res_hi, sums[0], krls);
    const bool ok = hi[0] > 0.0 && hi[1] > 0.0 && hi[1] - lo[1] < hi[0] - lo[0] && res_lo >= 0.0 && res_hi <= CAP;
    chk(both[1], elmk_routing_reservoir_clear(both[1]), "elmk_routing_reservoir_clear");  // (elmk_routing_clear would free it as well)
    for (int k = 0; k < 2; k++) {
      chk(both[k], elmk_routing_clear(both[k]), "elmk_routing_clear");
      chk(both[k], elmk_destroy(both[k]), "elmk_destroy");
    }
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "reservoir_demo: %s\n", e.what());
    return 1;
  }
}
