// irrigation_supply_demo.cc - the irrigation's river supply limit of elmk.h ("irrigation: river supply limit") through the C ABI: one
// crop cell of four dry columns on a small channel through two days of half-hour steps, once without the limit and once with it.
// Only the irrigation stage and the runoff routing run; the soil is not stepped, so every morning's check measures the same deficit,
// and no runoff is generated, so the channel only loses what the irrigation withdraws.  The channel holds 60 % of one day's demand.
// Without the limit the columns irrigate as if the river were full and VOLR goes negative.  With it the first two columns, which check
// at 06:00 and ask for half the day's demand, are granted in full; the other two check half an hour later and are cut back to what the
// first two have left (RATIO < 1); the second morning finds the channel nearly empty, and VOLR stays positive.
// The soil grid and the upload helpers come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/irrigation_supply_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o irrigation_supply_demo
//   ./irrigation_supply_demo
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

static void put_int(elmk_ctx* ctx, const char* name, int64_t n, int32_t v)
{
  std::vector<int32_t> a((size_t)n, v);
  chk(ctx, elmk_upload(ctx, fid(name), a.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), name);
}

// two days; returns the lowest VOLR seen.  volr0 < 0: the channel is given 60 % of the demand the first check measures
static double two_days(bool limit, double* volr0)
{
  const int64_t n = 4;
  const double dt = 1800.0, area = 1.0e8;
  const int nsteps = 96, vtype = 17;
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(n, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 2 /* crop */, 1, vtype, 0, 0), "elmk_set_land");
  std::vector<double> psn((size_t)ELMK_MXPFT * ELMK_PSN_NPARAM, 0.0), alb((size_t)ELMK_MXPFT * ELMK_ALB_NPARAM, 0.0), z0mr(ELMK_MXPFT, 0.0),
      displar(ELMK_MXPFT, 0.0);
  for (int p = 0; p < ELMK_MXPFT; p++) psn[(size_t)p * ELMK_PSN_NPARAM + 24] = -66000.0;  // smpso: all the stage reads of the tables
  chk(ctx, elmk_set_pft(ctx, psn.data(), alb.data(), z0mr.data(), displar.data()), "elmk_set_pft");
  // of the loam column the stage reads the layer thickness, the water and the retention curve; the soil is not stepped
  std::vector<double> zi, dz, z, liq(20, 0.0), rootfr(15, 0.0);
  soil_grid(zi, dz, z);
  for (int j = 0; j < 15; j++) liq[5 + j] = 0.25 * WATSAT * dz[5 + j] * 1000.0;  // a quarter saturated
  const double roots[6] = {0.3, 0.25, 0.2, 0.12, 0.08, 0.05};
  for (int j = 0; j < 6; j++) rootfr[j] = roots[j];
  put(ctx, "dz", n, dz);
  put(ctx, "h2osoi_liq", n, liq);
  put(ctx, "t_soisno", n, std::vector<double>(20, 290.0));
  put(ctx, "eff_porosity", n, std::vector<double>(15, WATSAT));
  put(ctx, "sucsat", n, std::vector<double>(15, SUCSAT));
  put(ctx, "bsw", n, std::vector<double>(15, BSW));
  put(ctx, "rootfr", n, rootfr);
  put(ctx, "elai", n, {2.0});
  put(ctx, "btran", n, {0.3});  // stressed
  put_int(ctx, "frac_veg_nosno", n, 1);
  put_int(ctx, "vtype", n, vtype);

  // the routing reads the water balance's QRUNOFF row (zeros here: nothing runs off), which needs the soil hydrology's rows
  chk(ctx, elmk_soil_hydrology_enable(ctx), "elmk_soil_hydrology_enable");
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-9), "elmk_water_balance_enable");
  // one output cell: the mean of the four columns
  const int64_t ptr[2] = {0, n};
  const int32_t col[4] = {0, 1, 2, 3};
  const double w[4] = {0.25, 0.25, 0.25, 0.25};
  chk(ctx, elmk_set_output_grid(ctx, 1, ptr, col, w, 0.0), "elmk_set_output_grid");
  const int32_t down[1] = {-1};
  const double ddist[1] = {1.0e9};  // an outlet that releases 5e-6 of its storage in a four-hour window
  chk(ctx, elmk_routing_enable(ctx, 1, down, ddist, &area, 0.35, 1), "elmk_routing_enable");
  // columns 0 and 1 pass 06:00 local at 06:00 UTC, columns 2 and 3 half an hour later
  const int32_t sched[4] = {0, 0, 84600, 84600};
  chk(ctx, elmk_irrigation_enable(ctx, sched), "elmk_irrigation_enable");
  chk(ctx, elmk_routing_set_withdrawal(ctx, 1), "elmk_routing_set_withdrawal");
  if (limit) chk(ctx, elmk_irrigation_supply_enable(ctx, 0.1), "elmk_irrigation_supply_enable");

  std::vector<double> rate(n), nleft(n);
  double volr = 0.0, ratio = 1.0, lowest = 1.0e300;
  bool filled = *volr0 >= 0.0;
  if (filled) chk(ctx, elmk_routing_init(ctx, volr0, nullptr, 0), "elmk_routing_init");
  std::printf("%s the limit\n%4s %6s %12s %12s %6s %8s %14s\n", limit ? "with" : "without", "step", "UTC", "RATE[0] mm/s", "RATE[2] mm/s", "NLEFT",
              "RATIO", "VOLR m3");
  for (int s = 0; s < nsteps; s++) {
    const int tod = (int)((long long)s * (long long)dt % 86400);
    chk(ctx, elmk_irrigation(ctx, dt, tod), "elmk_irrigation");
    chk(ctx, elmk_irrigation_read(ctx, ELMK_IRR_RATE, rate.data(), 0, n), "read");
    chk(ctx, elmk_irrigation_read(ctx, ELMK_IRR_NLEFT, nleft.data(), 0, n), "read");
    if (!filled && nleft[0] == 8.0) {  // the first check of the run without the limit: size the channel from what it asked for
      *volr0 = 0.6 * (rate[0] * dt * 8.0 * 0.001 * area);  // (all four columns ask for the same)
      chk(ctx, elmk_routing_init(ctx, volr0, nullptr, 0), "elmk_routing_init");
      filled = true;
    }
    chk(ctx, elmk_routing(ctx, dt), "elmk_routing");
    chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_VOLR, &volr, 0, 1), "read");
    if (limit) chk(ctx, elmk_irrigation_supply_read(ctx, ELMK_IRRSUP_RATIO, &ratio, 0, 1), "read");
    if (filled && volr < lowest) lowest = volr;
    if (tod >= 5 * 3600 + 1800 && tod <= 11 * 3600)
      std::printf("%4d %3d:%02d %12.5e %12.5e %6.0f %8.5f %14.6e\n", s, tod / 3600, tod % 3600 / 60, rate[0], rate[2], nleft[0], ratio, volr);
  }
  if (limit) {
    double unmet = 0.0;
    chk(ctx, elmk_irrigation_supply_read(ctx, ELMK_IRRSUP_UNMET_SUM, &unmet, 0, 1), "read");
    std::printf("unmet demand: %.6e m3\n", unmet);
  }
  std::printf("lowest VOLR: %.6e m3\n", lowest);
  chk(ctx, elmk_destroy(ctx), "elmk_destroy");
  return lowest;
}

int main()
{
  try {
    double volr0 = -1.0;
    const double without = two_days(false, &volr0);
    const double with = two_days(true, &volr0);
    return without < 0.0 && with > 0.0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "irrigation_supply_demo: %s\n", e.what());
    return 1;
  }
}
