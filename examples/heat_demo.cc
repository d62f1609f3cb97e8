// heat_demo.cc - a cold tributary joining a warm river (elmk.h "stream temperature"), through the C ABI: five cells, one uniform loam
// column per cell, a summer day of 48 half-hour steps.  Cells 0 -> 1 -> 2 -> 3 are the river, under the sun over warm ground; cell 4 is a
// shaded tributary over cold ground that joins the river in cell 2.  Every step uploads the hour's air and radiation, steps the
// hydrology and the water balance and routes the runoff with the HEAT form; prints the main channel's temperature above the
// confluence (cell 1), in the tributary (cell 4) and below the confluence (cell 2) per step, then the day's heat budget (H7).  In a
// model run elmk_run with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING does all of it on the device.  The columns,
// the cells and the kinematic scheme come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/heat_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o heat_demo
//   ./heat_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

// one value per column on each of nlev levels, [column][level]
static void put_cols(elmk_ctx* ctx, const char* name, const std::vector<double>& cols, int nlev = 1)
{
  std::vector<double> a(cols.size() * (size_t)nlev);
  for (size_t c = 0; c < cols.size(); c++)
    for (int l = 0; l < nlev; l++) a[c * (size_t)nlev + (size_t)l] = cols[c];
  chk(ctx, elmk_upload(ctx, fid(name), a.data(), 0, (int64_t)cols.size(), ELMK_LAYOUT_COL_MAJOR), name);
}

static const int64_t N = 5;  // columns = cells
static const int NSUB = 4;
static const int64_t ABOVE = 1, BELOW = 2, TRIB = 4;

static elmk_ctx* make()
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.7);
  hydrology_on(ctx, N, 2.0e-3);
  hydrology_start(ctx, N, 1.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, {1, 2, 3, -1, 2}, NSUB);  // the river 0 -> 1 -> 2 -> 3, the tributary 4 -> 2
  // a hillslope of 5 % with rough ground, 100 km of 10 m tributaries, a 2 km main channel 100 m wide
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e3, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  // the subsurface runoff carries the temperature of the third soil layer; the tributary runs under trees
  std::vector<double> shade(N, 0.1);
  shade[TRIB] = 1.0;
  chk(ctx, elmk_routing_heat_enable(ctx, 2, shade.data()), "elmk_routing_heat_enable");
  std::vector<double> t0(N, 293.0);
  t0[TRIB] = 279.0;
  chk(ctx, elmk_routing_heat_init(ctx, t0.data(), t0.data()), "elmk_routing_heat_init");
  // the ground: warm under the river's cells, cold under the tributary's
  std::vector<double> ground(N, 296.0);
  ground[TRIB] = 278.0;
  put_cols(ctx, "t_grnd", ground);
  put_cols(ctx, "t_soisno", ground, 20);
  return ctx;
}

int main()
{
  elmk_ctx* ctx = nullptr;
  try {
    const double dt = 1800.0, pi = 3.14159265358979;
    const int nsteps = 48;
    ctx = make();
    std::printf("a summer day of %d steps of %.0f s: the main channel's temperature above the confluence, in the cold tributary and below, K\n",
                nsteps, dt);
    std::printf("%4s %12s %12s %12s %12s\n", "step", "above", "tributary", "below", "sun W/m2");
    double heat_prev = 0.0, resid = 0.0, scale = 0.0;  // (a cold start holds no water, so no heat)
    bool ok = true;
    for (int s = 0; s < nsteps; s++) {
      const double hour = 0.5 * s, sun = std::fmax(0.0, std::sin(pi * (hour - 6.0) / 12.0));
      const double rain = 1.0e-3;
      std::vector<double> air(N, 291.0 + 8.0 * std::sin(pi * (hour - 9.0) / 12.0));
      air[TRIB] -= 9.0;  // the tributary's valley stays cool
      put_cols(ctx, "forc_tbot", air);
      put(ctx, "forc_pbot", N, {1.0e5});
      put(ctx, "forc_qbot", N, {8.0e-3});
      put(ctx, "forc_lwrad", N, {360.0});
      put(ctx, "forc_u", N, {2.0});
      put(ctx, "forc_v", N, {1.0});
      put(ctx, "forc_solad", N, {300.0 * sun, 260.0 * sun});
      put(ctx, "forc_solai", N, {70.0 * sun, 60.0 * sun});
      put(ctx, "qflx_top_soil", N, {rain});
      put(ctx, "forc_rain", N, {rain});
      chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
      chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
      chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      chk(ctx, elmk_water_balance(ctx, dt, nullptr, nullptr, nullptr), "elmk_water_balance");
      chk(ctx, elmk_routing(ctx, dt), "elmk_routing");  // the HEAT form while the extension is on
      double tr[N], sums[5];
      chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_TR, tr, 0, N), "elmk_routing_read");
      chk(ctx, elmk_routing_heat_budget(ctx, sums), "elmk_routing_heat_budget");
      resid += (sums[0] - heat_prev) - (sums[1] + sums[2] + sums[3] - sums[4]);
      scale = std::fmax(scale, std::fabs(sums[0]));
      heat_prev = sums[0];
      std::printf("%4d %12.6f %12.6f %12.6f %12.2f\n", s, tr[ABOVE], tr[TRIB], tr[BELOW], 690.0 * sun);
      if (s >= nsteps / 2) ok = ok && tr[TRIB] < tr[BELOW] && tr[BELOW] < tr[ABOVE];
    }
    std::printf("budget: closes to %.3e of the heat content (%.6e K m3)\n", scale > 0.0 ? std::fabs(resid) / scale : 0.0, scale);
    ok = ok && scale > 0.0 && std::fabs(resid) <= 1.0e-9 * scale;
    chk(ctx, elmk_routing_heat_clear(ctx), "elmk_routing_heat_clear");  // (elmk_routing_clear would free it as well)
    chk(ctx, elmk_routing_clear(ctx), "elmk_routing_clear");
    chk(ctx, elmk_destroy(ctx), "elmk_destroy");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "heat_demo: %s\n", e.what());
    return 1;
  }
}
