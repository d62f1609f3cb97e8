// soil_hydrology_demo.cc - the soil hydrology stage of elmk.h ("soil hydrology") on its own, through the C ABI: a day of half-hour
// steps of steady rain and root uptake on uniform loam columns that differ only in the depth of their water table.  No other physics
// runs, so the fluxes the stage reads (qflx_top_soil, qflx_rootsoi) are simply uploaded once; in a model run elmk_advance_physics
// writes them every step and elmk_run with ELMK_RUN_HYDROLOGY runs the stage after it.  Prints, per column, the water table, the
// aquifer, the surface store and the soil water at the start and the end, with the day's budget: the change of the stores against
// (rain - runoff - uptake - drainage) dt summed over the steps.  The columns come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/soil_hydrology_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o soil_hydrology_demo
//   ./soil_hydrology_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

static double soil_water(int64_t c, const std::vector<double>& liq)
{
  double s = 0.0;
  for (int j = 0; j < ELMK_HYD_NLAYER; j++) s += liq[(size_t)c * 20 + 5 + j];
  return s;
}

int main()
{
  try {
    const int64_t n = 6;
    const double dt = 1800.0, rain = 2.0e-3 /* mm/s: 7.2 mm/h */, uptake = 2.0e-5;
    const int nsteps = 48;
    elmk_ctx* ctx = nullptr;
    chk(ctx, elmk_create(n, 0, &ctx), "elmk_create");
    chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
    loam_columns(ctx, n, 0.5);  // half saturated
    std::vector<double> root(15, 0.0);
    for (int j = 0; j < 5; j++) root[j] = uptake / 5.0;
    put(ctx, "qflx_rootsoi", n, root);
    put(ctx, "qflx_top_soil", n, {rain});
    // (snl, h2osfc, frac_h2osfc, frac_sno_eff and the evaporation and dew terms stay at the zeros the context starts with)

    hydrology_on(ctx, n, 5.0e-3);
    const double depth[n] = {0.05, 0.5, 1.5, 3.0, 6.0, 0.0 /* cold start */};
    std::vector<double> zwt0(depth, depth + n), wa0(n, 4000.0), cold(n);
    chk(ctx, elmk_soil_hydrology_init(ctx, nullptr, nullptr), "init(cold start)");
    chk(ctx, elmk_soil_hydrology_read(ctx, ELMK_HYD_ZWT, cold.data(), 0, n), "read");
    zwt0[n - 1] = cold[n - 1];
    chk(ctx, elmk_soil_hydrology_init(ctx, zwt0.data(), wa0.data()), "init");

    std::vector<double> liq0((size_t)n * 20), liq1((size_t)n * 20), h2osfc(n), zwt(n), wa(n), row(n), out(n, 0.0);
    chk(ctx, elmk_download(ctx, fid("h2osoi_liq"), liq0.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
    for (int s = 0; s < nsteps; s++) {
      chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      for (int which : {ELMK_HYD_QFLX_SURF, ELMK_HYD_QFLX_H2OSFC_SURF, ELMK_HYD_QFLX_DRAIN}) {
        chk(ctx, elmk_soil_hydrology_read(ctx, which, row.data(), 0, n), "read");
        for (int64_t c = 0; c < n; c++) out[c] += row[c] * dt;
      }
    }
    chk(ctx, elmk_download(ctx, fid("h2osoi_liq"), liq1.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
    chk(ctx, elmk_download(ctx, fid("h2osfc"), h2osfc.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
    chk(ctx, elmk_soil_hydrology_read(ctx, ELMK_HYD_ZWT, zwt.data(), 0, n), "read");
    chk(ctx, elmk_soil_hydrology_read(ctx, ELMK_HYD_WA, wa.data(), 0, n), "read");

    std::printf("soil hydrology, %d steps of %.0f s, rain %.1f mm, uptake %.2f mm\n", nsteps, dt, rain * dt * nsteps, uptake * dt * nsteps);
    std::printf("%6s %9s %9s %10s %10s %9s %9s %10s %11s\n", "column", "zwt0 m", "zwt m", "soil0 mm", "soil mm", "h2osfc", "wa - wa0", "runoff mm", "budget mm");
    double worst = 0.0;
    for (int64_t c = 0; c < n; c++) {
      const double stores = (soil_water(c, liq1) - soil_water(c, liq0)) + h2osfc[c] + (wa[c] - wa0[c]);
      const double budget = stores - ((rain - uptake) * dt * nsteps - out[c]);
      worst = std::fmax(worst, std::fabs(budget));
      std::printf("%6lld %9.3f %9.3f %10.2f %10.2f %9.3f %9.3f %10.3f %11.2e\n", (long long)c, zwt0[c], zwt[c], soil_water(c, liq0),
                  soil_water(c, liq1), h2osfc[c], wa[c] - wa0[c], out[c], budget);
    }
    chk(ctx, elmk_destroy(ctx), "elmk_destroy");
    return worst < 1.0e-8 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "soil_hydrology_demo: %s\n", e.what());
    return 1;
  }
}
