// permafrost_hydrology_demo.cc - the frost table and the perched water table of elmk.h ("soil hydrology", F') through the C ABI: a few
// half-hour steps on five wet loam columns over permafrost whose thaw front starts at layers 3 .. 7 and moves one layer down half way.
// Columns 0, 2 and 4 start with their water table above the frost table (branch A: the water table itself drains laterally; in the
// shallow column 0 it falls through the frost table at once), columns 1 and 3 with it far below (branch B: where a saturated zone is
// perched over the frozen layers, it drains).  No other physics runs, so the soil temperature is simply uploaded; in a model run
// elmk_advance_physics writes it and elmk_run with ELMK_RUN_HYDROLOGY | ELMK_RUN_ALT runs both features.
// Prints, per step and column, the active layer thickness (elmk_active_layer_*), the frost table, the perched water table and the
// perched drainage.  The columns come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/permafrost_hydrology_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o permafrost_hydrology_demo
//   ./permafrost_hydrology_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

int main()
{
  try {
    const int64_t n = 5;
    const double dt = 1800.0, pi = 3.14159265358979323846;
    const int nsteps = 4;
    elmk_ctx* ctx = nullptr;
    chk(ctx, elmk_create(n, 0, &ctx), "elmk_create");
    chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
    std::vector<double> lat(n, 70.0 * pi / 180.0), lon(n, 0.0);
    chk(ctx, elmk_set_column_geography(ctx, lat.data(), lon.data()), "elmk_set_column_geography");
    loam_columns(ctx, n, 0.96);  // melt water on the frozen layers
    std::vector<double> zi, dz, z, liq(20, 0.0);
    soil_grid(zi, dz, z);
    for (int j = 0; j < 15; j++) liq[5 + j] = (j < 2 ? 0.5 : 0.96) * WATSAT * dz[5 + j] * 1000.0;  // under two drier layers on top
    put(ctx, "h2osoi_liq", n, liq);

    chk(ctx, elmk_active_layer_enable(ctx), "elmk_active_layer_enable");
    const double slope = 3.0 * pi / 180.0;
    hydrology_on(ctx, n, 5.0e-3, 0.4, /*k_wet=*/std::sin(slope), /*rsub=*/10.0 * std::sin(slope));
    std::vector<double> q_perch_max(n, 1.0e-5 * std::sin(slope));
    chk(ctx, elmk_soil_hydrology_frost_enable(ctx, q_perch_max.data()), "elmk_soil_hydrology_frost_enable");
    std::vector<double> zwt0(n), wa0(n, 4000.0);
    for (int64_t c = 0; c < n; c++) zwt0[c] = c % 2 == 0 ? 0.5 * z[5 + 3 + c] : 6.0;
    chk(ctx, elmk_soil_hydrology_init(ctx, zwt0.data(), wa0.data()), "elmk_soil_hydrology_init");

    std::printf("permafrost hydrology, %d steps of %.0f s, %lld columns, q_perch_max %.3e 1/s\n", nsteps, dt, (long long)n, q_perch_max[0]);
    std::printf("%4s %6s %9s %14s %14s %22s\n", "step", "column", "ALT m", "FROST_TABLE m", "ZWT_PERCHED m", "QFLX_DRAIN_PERCHED mm/s");
    std::vector<double> t((size_t)n * 20), alt(n), ft(n), zwp(n), qp(n);
    bool ok = true;
    double drained = 0.0;
    for (int s = 0; s < nsteps; s++) {
      for (int64_t c = 0; c < n; c++) {
        const int front = 3 + (int)c + (s >= nsteps / 2 ? 1 : 0);  // the first frozen layer
        for (int l = 0; l < 20; l++) t[(size_t)c * 20 + l] = l - 5 < front ? 274.15 + 0.1 * (front - (l - 5)) : 272.15;
      }
      chk(ctx, elmk_upload(ctx, fid("t_soisno"), t.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "t_soisno");
      chk(ctx, elmk_active_layer_update(ctx, 0), "elmk_active_layer_update");
      chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      chk(ctx, elmk_active_layer_read(ctx, ELMK_ALT_ALT, alt.data(), 0, n), "read");
      chk(ctx, elmk_soil_hydrology_frost_read(ctx, ELMK_HYDF_FROST_TABLE, ft.data(), 0, n), "read");
      chk(ctx, elmk_soil_hydrology_frost_read(ctx, ELMK_HYDF_ZWT_PERCHED, zwp.data(), 0, n), "read");
      chk(ctx, elmk_soil_hydrology_frost_read(ctx, ELMK_HYDF_QFLX_DRAIN_PERCHED, qp.data(), 0, n), "read");
      for (int64_t c = 0; c < n; c++) {
        std::printf("%4d %6lld %9.4f %14.4f %14.4f %22.6e\n", s, (long long)c, alt[c], ft[c], zwp[c], qp[c]);
        // the thaw depth lies between the last thawed node and the first frozen one, which is the frost table
        ok = ok && std::isfinite(alt[c]) && std::isfinite(ft[c]) && std::isfinite(zwp[c]) && std::isfinite(qp[c]) && alt[c] <= ft[c] &&
             zwp[c] <= ft[c] && qp[c] >= 0.0;
        drained += qp[c] * dt;
      }
    }
    chk(ctx, elmk_destroy(ctx), "elmk_destroy");
    return ok && drained > 0.0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "permafrost_hydrology_demo: %s\n", e.what());
    return 1;
  }
}
