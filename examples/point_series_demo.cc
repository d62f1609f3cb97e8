// point_series_demo.cc - the two outputs a modeller looks at first, through the C ABI (elmk.h "point series"): the hydrograph at a gauge
// cell and the per-step series at a few columns.  The storm of kinematic_routing_demo.cc on its chain of eight cells, a day of 48
// half-hour steps in two windows of 24.  Three columns (the water table ZWT and the top soil layer's liquid water) and the outlet cell
// (QOUT and VOLR) are named once; after every step ONE launch, elmk_points_record, gathers their current values into a ring on the
// device, stamped with the step's time, and nothing is downloaded until the day is over.  A twin context takes the same steps and
// downloads after each one what the series should hold - elmk_routing_read for the cell rows, elmk_soil_hydrology_read and
// elmk_download for the columns; the demo prints the hydrograph and "OK" when the series agrees with the twin in every bit.
// The steps are the stand-alone calls; in a model run elmk_points_set_run(ctx, 1) makes every step of elmk_run record by itself, after
// the routing and the history, with the step's decday as the stamp.  The columns, the cells and the kinematic scheme come from
// examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/point_series_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o point_series_demo
//   ./point_series_demo
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 8;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4, NSTEPS = 48, WINDOW = 24, STORM_STEPS = 12;
static const double DT = 1800.0, STORM = 4.0e-3 /* mm/s: 14.4 mm/h */;
static const int64_t COLUMNS[3] = {0, 4, 7}, GAUGE[1] = {N - 1};
enum { ZWT, LIQ, QOUT, VOLR, NENTRY };

static elmk_ctx* make()
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.7);
  hydrology_on(ctx, N, 2.0e-3);
  hydrology_start(ctx, N, 1.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, chain(N), NSUB);
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  return ctx;
}

static void step(elmk_ctx* ctx, int s)
{
  const double rain = s < STORM_STEPS ? STORM : 0.0;
  put(ctx, "qflx_top_soil", N, {rain});
  put(ctx, "forc_rain", N, {rain});
  chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
  chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
  chk(ctx, elmk_soil_hydrology(ctx, DT), "elmk_soil_hydrology");
  chk(ctx, elmk_water_balance(ctx, DT, nullptr, nullptr, nullptr), "elmk_water_balance");
  chk(ctx, elmk_routing(ctx, DT), "elmk_routing");
}

// what the series should hold after a step, by the download calls: ZWT[3], the top soil layer's liquid water[3], QOUT, VOLR
static void downloads(elmk_ctx* ctx, double out[8])
{
  std::vector<double> row((size_t)N), liq((size_t)20 * N);
  chk(ctx, elmk_soil_hydrology_read(ctx, ELMK_HYD_ZWT, row.data(), 0, N), "elmk_soil_hydrology_read");
  chk(ctx, elmk_download(ctx, fid("h2osoi_liq"), liq.data(), 0, N, ELMK_LAYOUT_COL_MAJOR), "elmk_download");
  for (int k = 0; k < 3; k++) {
    out[k] = row[(size_t)COLUMNS[k]];
    out[3 + k] = liq[(size_t)COLUMNS[k] * 20 + 5];
  }
  chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_QOUT, row.data(), 0, N), "elmk_routing_read");
  out[6] = row[(size_t)GAUGE[0]];
  chk(ctx, elmk_routing_read(ctx, ELMK_ROUTE_VOLR, row.data(), 0, N), "elmk_routing_read");
  out[7] = row[(size_t)GAUGE[0]];
}

int main()
{
  try {
    // the context that records
    elmk_ctx* A = make();
    int entry[NENTRY];
    chk(A, elmk_points_set(A, ELMK_POINTS_COLUMNS, 3, COLUMNS), "elmk_points_set");
    chk(A, elmk_points_set(A, ELMK_POINTS_CELLS, 1, GAUGE), "elmk_points_set");
    chk(A, entry[ZWT] = elmk_points_add_row(A, ELMK_ROWS_HYDROLOGY, ELMK_HYD_ZWT), "elmk_points_add_row");
    chk(A, entry[LIQ] = elmk_points_add_field(A, fid("h2osoi_liq"), 5), "elmk_points_add_field");
    chk(A, entry[QOUT] = elmk_points_add_cell_row(A, ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_QOUT), "elmk_points_add_cell_row");
    chk(A, entry[VOLR] = elmk_points_add_cell_row(A, ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_VOLR), "elmk_points_add_cell_row");
    chk(A, elmk_points_reserve(A, NSTEPS), "elmk_points_reserve");
    for (int window = 0; window < NSTEPS / WINDOW; window++)  // nothing comes back to the host between the steps
      for (int s = window * WINDOW; s < (window + 1) * WINDOW; s++) {
        step(A, s);
        chk(A, elmk_points_record(A, 1.0 + (s + 1) * DT / 86400.0), "elmk_points_record");
      }
    int64_t total = 0, held = 0;
    chk(A, elmk_points_count(A, &total, &held), "elmk_points_count");
    std::vector<double> stamps((size_t)NSTEPS), zwt((size_t)NSTEPS * 3), liq((size_t)NSTEPS * 3), qout((size_t)NSTEPS), volr((size_t)NSTEPS);
    chk(A, elmk_points_stamps(A, stamps.data(), 0, NSTEPS), "elmk_points_stamps");
    chk(A, elmk_points_read(A, entry[ZWT], zwt.data(), 0, NSTEPS), "elmk_points_read");
    chk(A, elmk_points_read(A, entry[LIQ], liq.data(), 0, NSTEPS), "elmk_points_read");
    chk(A, elmk_points_read(A, entry[QOUT], qout.data(), 0, NSTEPS), "elmk_points_read");
    chk(A, elmk_points_read(A, entry[VOLR], volr.data(), 0, NSTEPS), "elmk_points_read");
    chk(A, elmk_points_clear(A), "elmk_points_clear");  // (the entries hold the routing's rows)
    chk(A, elmk_routing_clear(A), "elmk_routing_clear");
    chk(A, elmk_destroy(A), "elmk_destroy");

    // the twin: the same steps, a download after each
    elmk_ctx* B = make();
    bool same = total == NSTEPS && held == NSTEPS;
    double peak = 0.0;
    std::printf("the hydrograph at the outlet of a chain of %lld cells, a storm of %.1f mm in the first %d of %d steps of %.0f s\n", (long long)N,
                STORM * DT * STORM_STEPS, STORM_STEPS, NSTEPS, DT);
    std::printf("%4s %10s %14s %14s %12s\n", "step", "day", "QOUT m3/s", "VOLR m3", "ZWT[0] m");
    for (int s = 0; s < NSTEPS; s++) {
      step(B, s);
      double want[8];
      downloads(B, want);
      const double got[8] = {zwt[(size_t)s * 3], zwt[(size_t)s * 3 + 1], zwt[(size_t)s * 3 + 2], liq[(size_t)s * 3], liq[(size_t)s * 3 + 1],
                             liq[(size_t)s * 3 + 2], qout[(size_t)s], volr[(size_t)s]};
      same = same && std::memcmp(got, want, sizeof got) == 0 && stamps[(size_t)s] == 1.0 + (s + 1) * DT / 86400.0;
      peak = qout[(size_t)s] > peak ? qout[(size_t)s] : peak;
      if (s % 4 == 3) std::printf("%4d %10.5f %14.6e %14.6e %12.6f\n", s, stamps[(size_t)s], qout[(size_t)s], volr[(size_t)s], zwt[(size_t)s * 3]);
    }
    chk(B, elmk_routing_clear(B), "elmk_routing_clear");
    chk(B, elmk_destroy(B), "elmk_destroy");
    const bool sane = peak > 0.0;
    std::printf("%s\n", same && sane ? "OK: the series holds what the twin downloaded after every step, in every bit"
                                     : "DIFFERENT: the series does not hold what the twin downloaded");
    return same && sane ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "point_series_demo: %s\n", e.what());
    return 1;
  }
}
