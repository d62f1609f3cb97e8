// water_balance_demo.cc - the closed water budget of elmk.h ("water balance") and history entries over feature rows, through the C ABI:
// a day of half-hour steps of steady rain and root uptake on the uniform loam columns of examples/demo_site.h.  Every step runs
// elmk_init_timestep, elmk_water_balance_begin (W0), the soil hydrology stage and elmk_water_balance (W1 - W8), and samples a history
// tape that averages two feature rows: total runoff QRUNOFF (a water-balance row) and the water table ZWT (a hydrology row).  Prints
// the worst |ERRH2O| and the number of columns over the tolerance per step, then the tape means per column.  In a model run elmk_run
// with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_HISTORY does all of it on the device.
//
//   g++ -std=c++17 -Iinclude examples/water_balance_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o water_balance_demo
//   ./water_balance_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

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
    // what the budget sees of the same fluxes: the rain that reaches the ground and the uptake that leaves as transpiration
    put(ctx, "forc_rain", n, {rain});
    put(ctx, "qflx_evap_tot", n, {uptake});
    // (snl, h2osfc, frac_h2osfc, frac_sno_eff and the evaporation and dew terms stay at the zeros the context starts with)

    hydrology_on(ctx, n, 5.0e-3);
    const double depth[n] = {0.05, 0.5, 1.5, 3.0, 6.0, 0.0 /* cold start */};
    std::vector<double> zwt0(depth, depth + n), wa0(n, 4000.0), cold(n);
    chk(ctx, elmk_soil_hydrology_init(ctx, nullptr, nullptr), "init(cold start)");
    chk(ctx, elmk_soil_hydrology_read(ctx, ELMK_HYD_ZWT, cold.data(), 0, n), "read");
    zwt0[n - 1] = cold[n - 1];
    chk(ctx, elmk_soil_hydrology_init(ctx, zwt0.data(), wa0.data()), "init");

    const double tol = 1.0e-8;  // mm
    chk(ctx, elmk_water_balance_enable(ctx, tol), "elmk_water_balance_enable");
    const int e_runoff = elmk_column_history_add_row(ctx, 0, ELMK_ROWS_WATER_BALANCE, ELMK_WB_QRUNOFF, ELMK_HIST_AVG);
    chk(ctx, e_runoff, "elmk_column_history_add_row(QRUNOFF)");
    const int e_zwt = elmk_column_history_add_row(ctx, 0, ELMK_ROWS_HYDROLOGY, ELMK_HYD_ZWT, ELMK_HIST_AVG);
    chk(ctx, e_zwt, "elmk_column_history_add_row(ZWT)");

    std::printf("water balance, %d steps of %.0f s, rain %.1f mm, uptake %.2f mm, tolerance %.1e mm\n", nsteps, dt, rain * dt * nsteps,
                uptake * dt * nsteps, tol);
    std::printf("%4s %14s %6s %10s\n", "step", "worst |ERRH2O|", "nbad", "first bad");
    double worst = 0.0;
    int64_t bad_total = 0;
    for (int s = 0; s < nsteps; s++) {
      double mms[3][3];
      int64_t nbad = 0, first = -1;
      chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
      chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
      chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      chk(ctx, elmk_water_balance(ctx, dt, &mms[0][0], &nbad, &first), "elmk_water_balance");
      chk(ctx, elmk_history_accumulate(ctx), "elmk_history_accumulate");
      const double w = std::fmax(std::fabs(mms[0][0]), std::fabs(mms[0][1]));  // triple 0: (min, max, sum) of ERRH2O
      worst = std::fmax(worst, w);
      bad_total += nbad;
      std::printf("%4d %14.3e %6lld %10lld\n", s, w, (long long)nbad, (long long)first);
    }
    std::vector<double> runoff(n), zwt(n), tws(n);
    chk(ctx, elmk_history_read(ctx, e_runoff, runoff.data(), 0, n, ELMK_LAYOUT_SOA), "elmk_history_read");
    chk(ctx, elmk_history_read(ctx, e_zwt, zwt.data(), 0, n, ELMK_LAYOUT_SOA), "elmk_history_read");
    chk(ctx, elmk_water_balance_read(ctx, ELMK_WB_ENDWB, tws.data(), 0, n), "elmk_water_balance_read");
    std::printf("%6s %9s %16s %12s %12s\n", "column", "zwt0 m", "mean QRUNOFF mm/s", "mean ZWT m", "TWS mm");
    for (int64_t c = 0; c < n; c++) std::printf("%6lld %9.3f %16.6e %12.4f %12.3f\n", (long long)c, zwt0[c], runoff[c], zwt[c], tws[c]);
    chk(ctx, elmk_history_clear(ctx), "elmk_history_clear");
    chk(ctx, elmk_water_balance_clear(ctx), "elmk_water_balance_clear");
    chk(ctx, elmk_destroy(ctx), "elmk_destroy");
    return (worst < tol && bad_total == 0) ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "water_balance_demo: %s\n", e.what());
    return 1;
  }
}
