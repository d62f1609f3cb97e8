// river_output_demo.cc - what a river model is run for, through the library's own tapes and image (elmk.h "cell rows on history tapes"
// and "restart", version 6), through the C ABI: the storm of kinematic_routing_demo.cc on its chain of eight cells, routed by the
// kinematic-wave scheme with the floodplain inundation on.  Three cell-row entries sample the routing's result of every step on the
// device: the mean and the peak of QOUT and the maximum of FLOOD_FRAC.  The run is made twice: once in one piece, and once in two halves
// through a restart image that carries the river's state (ELMK_OPT_RESTART_CELLS) - the second half starts in a fresh context with no
// elmk_routing_init, elmk_routing_kinematic_init or elmk_routing_inundation_init call.  Prints each cell's mean and peak discharge and
// the largest flooded fraction of the whole run, and "identical" when the two runs agree in every bit of them.  The steps are the
// stand-alone calls; in a model run elmk_run with ELMK_RUN_HYDROLOGY | ELMK_RUN_WATER_BALANCE | ELMK_RUN_ROUTING | ELMK_RUN_HISTORY
// does the same on the device.  The columns, the cells and the kinematic scheme come from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/river_output_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o river_output_demo
//   ./river_output_demo
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_site.h"

using namespace demo;
static const int64_t N = 8;  // columns = cells: cell c drains into c + 1, the last is the outlet
static const int NSUB = 4, NSTEPS = 48, STORM_STEPS = 12;
static const double DT = 1800.0, STORM = 4.0e-3 /* mm/s: 14.4 mm/h */;
enum { MEAN_QOUT, PEAK_QOUT, MAX_FRAC, NENTRY };

// the river stages, the option and the three entries; `fresh`: the soil columns too (a restart takes them from the image)
static elmk_ctx* make(bool fresh, int entry[NENTRY])
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  if (fresh) loam_columns(ctx, N, 0.7);
  hydrology_on(ctx, N, 2.0e-3);
  if (fresh) hydrology_start(ctx, N, 1.0);
  chk(ctx, elmk_water_balance_enable(ctx, 1.0e-6), "elmk_water_balance_enable");
  river_cells(ctx, chain(N), NSUB);
  // kinematic_routing_demo.cc's cells under banks of 0.5 m and a floodplain that rises 0.2 m per tenth of the cell
  const double value[ELMK_KW_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  kinematic_on(ctx, N, value);
  std::vector<double> rdepth(N, 0.5), eprof((size_t)ELMK_FP_NPROF * N);
  for (int k = 0; k < ELMK_FP_NPROF; k++)
    for (int64_t c = 0; c < N; c++) eprof[(size_t)k * N + c] = 0.2 * k;
  chk(ctx, elmk_routing_inundation_enable(ctx, rdepth.data(), eprof.data()), "elmk_routing_inundation_enable");
  chk(ctx, elmk_set_option(ctx, ELMK_OPT_RESTART_CELLS, 1), "elmk_set_option");
  const int which[NENTRY] = {ELMK_ROUTE_QOUT, ELMK_ROUTE_QOUT, ELMK_ROUTE_FLOOD_FRAC}, op[NENTRY] = {ELMK_HIST_AVG, ELMK_HIST_MAX, ELMK_HIST_MAX};
  for (int k = 0; k < NENTRY; k++) {
    entry[k] = elmk_cell_history_add_row(ctx, 0, ELMK_CELL_ROWS_ROUTING, which[k], op[k]);
    chk(ctx, entry[k], "elmk_cell_history_add_row");
  }
  return ctx;
}

static void steps(elmk_ctx* ctx, int s0, int s1)
{
  for (int s = s0; s < s1; s++) {
    const double rain = s < STORM_STEPS ? STORM : 0.0;
    put(ctx, "qflx_top_soil", N, {rain});
    put(ctx, "forc_rain", N, {rain});
    chk(ctx, elmk_init_timestep(ctx), "elmk_init_timestep");
    chk(ctx, elmk_water_balance_begin(ctx), "elmk_water_balance_begin");
    chk(ctx, elmk_soil_hydrology(ctx, DT), "elmk_soil_hydrology");
    chk(ctx, elmk_water_balance(ctx, DT, nullptr, nullptr, nullptr), "elmk_water_balance");
    chk(ctx, elmk_routing(ctx, DT), "elmk_routing");
    chk(ctx, elmk_history_accumulate(ctx), "elmk_history_accumulate");  // the sample of step s: the routing's result of step s
  }
}

// [NENTRY][N], and the routing's call count
static std::vector<double> results(elmk_ctx* ctx, const int entry[NENTRY], int64_t* ncalls)
{
  std::vector<double> out((size_t)NENTRY * N);
  for (int k = 0; k < NENTRY; k++) chk(ctx, elmk_history_read(ctx, entry[k], out.data() + (size_t)k * N, 0, N, ELMK_LAYOUT_SOA), "elmk_history_read");
  chk(ctx, elmk_routing_count(ctx, ncalls), "elmk_routing_count");
  return out;
}

static void finish(elmk_ctx* ctx)
{
  chk(ctx, elmk_history_clear(ctx), "elmk_history_clear");  // (the entries hold the routing's rows)
  chk(ctx, elmk_routing_clear(ctx), "elmk_routing_clear");
  chk(ctx, elmk_destroy(ctx), "elmk_destroy");
}

int main()
{
  try {
    int entry[NENTRY];
    // the run that never stopped
    elmk_ctx* A = make(true, entry);
    steps(A, 0, NSTEPS);
    int64_t calls_a = 0, calls_c = 0;
    const std::vector<double> whole = results(A, entry, &calls_a);
    finish(A);
    // the first half, the image, a fresh context, the second half
    elmk_ctx* B = make(true, entry);
    steps(B, 0, NSTEPS / 2);
    int64_t bytes = 0;
    chk(B, elmk_restart_size(B, &bytes), "elmk_restart_size");
    std::vector<unsigned char> image((size_t)bytes);
    chk(B, elmk_restart_save(B, 0, image.data(), bytes), "elmk_restart_save");
    finish(B);
    uint32_t version = 0;
    std::memcpy(&version, image.data() + 8, 4);
    elmk_ctx* C = make(false, entry);  // enable the river stages, add the entries, load: no _init call
    chk(C, elmk_restart_load(C, 0, image.data(), bytes), "elmk_restart_load");
    steps(C, NSTEPS / 2, NSTEPS);
    const std::vector<double> halves = results(C, entry, &calls_c);
    finish(C);

    std::printf("a storm of %.1f mm in %d steps of %.0f s on a chain of %lld cells of 100 km2, %d steps; a version-%u image of %lld bytes after %d\n",
                STORM * DT * STORM_STEPS, STORM_STEPS, DT, (long long)N, NSTEPS, version, (long long)bytes, NSTEPS / 2);
    std::printf("%4s %16s %16s %16s\n", "cell", "mean QOUT m3/s", "peak QOUT m3/s", "max FLOOD_FRAC");
    double frac = 0.0;
    for (int64_t c = 0; c < N; c++) {
      std::printf("%4lld %16.6e %16.6e %16.6e\n", (long long)c, halves[MEAN_QOUT * N + c], halves[PEAK_QOUT * N + c], halves[MAX_FRAC * N + c]);
      frac = std::fmax(frac, halves[MAX_FRAC * N + c]);
    }
    std::printf("the largest flooded fraction of the run: %.6f\n", frac);
    const bool same = calls_a == NSTEPS && calls_c == NSTEPS && std::memcmp(whole.data(), halves.data(), whole.size() * sizeof(double)) == 0;
    const bool sane = version == (uint32_t)ELMK_RESTART_VERSION_ROUTING && halves[PEAK_QOUT * N + N - 1] > 0.0;
    std::printf("%s\n", same ? "identical: the two halves through the image give the bits of the run that never stopped"
                             : "DIFFERENT: the two halves do not give the run that never stopped");
    return same && sane ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "river_output_demo: %s\n", e.what());
    return 1;
  }
}
