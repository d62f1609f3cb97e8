// command_area_demo.cc - a dam that supplies a cell forty kilometres below it (elmk.h "command areas"), through the C ABI: a chain of
// four cells, one uniform loam column per cell, a reservoir of 1e9 m3 in cell 0 that holds its water back, and a crop cell 3 whose
// irrigation withdraws 50 m3/s through a dry season - more than its own channel carries.  Two contexts step the same columns through
// two days of hourly steps.  In the first the dam serves only its own cell: the crop cell's withdrawal drives its tributary store below
// zero.  In the second the crop cell hangs on the dam (share 1, claim 0.5): the dam gives what the cell asks, the cell's input is
// credited, and the store stays above zero while the reservoir falls.  Prints the crop cell's tributary store without and with the
// part, what the cell took and the reservoir's storage per step.  In a model run elmk_run with ELMK_RUN_IRRIGATION | ELMK_RUN_HYDROLOGY |
// ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING does all of it on the device.  The columns, the cells and the kinematic scheme come from
// examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/command_area_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o command_area_demo
//   ./command_area_demo
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 4;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4;
static const int64_t DAM = 0, CROP = 3;
static const double CAP = 1.0e9, RATE = 5.0e-4;  // mm/s over the crop cell's 100 km2: 50 m3/s

static elmk_ctx* make(bool command)
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.5);
  hydrology_on(ctx, N, 2.0e-3);
  hydrology_start(ctx, N, 3.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, chain(N), NSUB);
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  const std::vector<double> wt0(N, 1.0e4);  // a little water in the tributaries
  chk(ctx, elmk_routing_kinematic_init(ctx, nullptr, wt0.data()), "elmk_routing_kinematic_init");
  // the irrigation: no column follows a schedule; the crop column's window is open through the demo and applies RATE
  const std::vector<int32_t> sched(N, -1);
  std::vector<double> rate(N, 0.0), nleft(N, 0.0);
  rate[CROP] = RATE;
  nleft[CROP] = 1000.0;
  chk(ctx, elmk_irrigation_enable(ctx, sched.data()), "elmk_irrigation_enable");
  chk(ctx, elmk_irrigation_init(ctx, rate.data(), nleft.data()), "elmk_irrigation_init");
  chk(ctx, elmk_routing_set_withdrawal(ctx, 1), "elmk_routing_set_withdrawal");
  // the dam: BETA 1 and a target of 0 - it releases a tenth of its inflow and stores the rest
  std::vector<double> cap(N, 0.0), target((size_t)12 * N, 0.0), beta(N, 0.0), res(N, 0.0);
  const std::vector<int32_t> mstart(N, 0);
  cap[DAM] = CAP;
  beta[DAM] = 1.0;
  res[DAM] = 0.8 * CAP;
  chk(ctx, elmk_routing_reservoir_enable(ctx, cap.data(), target.data(), beta.data(), mstart.data()), "elmk_routing_reservoir_enable");
  chk(ctx, elmk_routing_reservoir_init(ctx, res.data(), nullptr), "elmk_routing_reservoir_init");
  if (command) {
    // dam[4][N] (-1 = empty slot), share[4][N], claim[4][N]: the crop cell asks all of its remaining withdrawal of the dam
    std::vector<int32_t> dam((size_t)ELMK_CMD_NDEP * N, -1);
    std::vector<double> share((size_t)ELMK_CMD_NDEP * N, 0.0), claim((size_t)ELMK_CMD_NDEP * N, 0.0);
    dam[CROP] = (int32_t)DAM;
    share[CROP] = 1.0;
    claim[CROP] = 0.5;
    chk(ctx, elmk_routing_command_enable(ctx, dam.data(), share.data(), claim.data()), "elmk_routing_command_enable");
  }
  return ctx;
}

int main()
{
  elmk_ctx* both[2] = {nullptr, nullptr};
  try {
    const double dt = 3600.0;
    const int nsteps = 48;
    both[0] = make(false);
    both[1] = make(true);
    std::printf("two days of hourly steps on a chain of %lld cells of 100 km2: a dam of %.1e m3 in cell %lld, a crop cell %lld that withdraws %.0f m3/s\n",
                (long long)N, CAP, (long long)DAM, (long long)CROP, RATE * 1.0e-3 * 1.0e8);
    std::printf("%4s %14s %14s %14s %14s\n", "step", "WT alone m3", "WT served m3", "TAKE m3", "RES m3");
    double lo[2] = {1e300, 1e300}, taken = 0.0, res = 0.0;
    bool falls = true, takes = true;
    double res_before = 0.8 * CAP;
    for (int s = 0; s < nsteps; s++) {
      double wt[2], take = 0.0;
      for (int k = 0; k < 2; k++) {
        elmk_ctx* ctx = both[k];
        put(ctx, "qflx_top_soil", N, {1.0e-6});
        put(ctx, "forc_rain", N, {1.0e-6});
        chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
        chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
        chk(ctx, elmk_irrigation(ctx, dt, (s * 3600) % 86400), "elmk_irrigation");
        chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
        chk(ctx, elmk_water_balance(ctx, dt, nullptr, nullptr, nullptr), "elmk_water_balance");
        chk(ctx, elmk_routing_reservoir_time(ctx, 6, 0), "elmk_routing_reservoir_time");
        chk(ctx, elmk_routing(ctx, dt), "elmk_routing");  // with the part on: the CMD form and the two launches behind it
        chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_WT, &wt[k], CROP, 1), "elmk_routing_read");
        if (wt[k] < lo[k]) lo[k] = wt[k];
      }
      chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_CMD_TAKE, &take, CROP, 1), "elmk_routing_read");
      chk(both[1], elmk_routing_read(both[1], ELMK_ROUTE_RES, &res, DAM, 1), "elmk_routing_read");
      taken += take;
      takes = takes && take > 0.0;
      falls = falls && res < res_before;
      res_before = res;
      std::printf("%4d %14.6e %14.6e %14.6e %14.6e\n", s, wt[0], wt[1], take, res);
    }
    double sums[2];
    chk(both[1], elmk_routing_command_budget(both[1], sums), "elmk_routing_command_budget");
    std::printf("alone:        the crop cell's tributary store falls to %.4e m3\n", lo[0]);
    std::printf("command area: it stays at or above %.4e m3; the cell took %.4e m3 in all, the dam gave %.4e m3 in the last step and holds %.4e m3\n",
                lo[1], taken, sums[0], res);
    const bool ok = lo[0] < 0.0 && lo[1] >= 0.0 && takes && falls;
    chk(both[1], elmk_routing_command_clear(both[1]), "elmk_routing_command_clear");  // (elmk_routing_clear would free it as well)
    for (int k = 0; k < 2; k++) {
      chk(both[k], elmk_routing_clear(both[k]), "elmk_routing_clear");
      chk(both[k], elmk_destroy(both[k]), "elmk_destroy");
    }
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "command_area_demo: %s\n", e.what());
    return 1;
  }
}
