// hillslope_demo.cc - the hillslope lateral flow of elmk.h ("hillslope lateral flow", L1 - L3) through the C ABI: five loam columns in a
// chain down a slope of 3 m per column, the toe (column 0) at the stream, under uniform rain, 96 half-hour steps, once with the
// extension and once without.  With it the columns pass groundwater downhill and the toe discharges to the stream: the toe ends wetter
// than the ridge.  Without it every column drains by its own baseflow and the five water tables stay equal.  No other physics runs.
// Prints, per step, the water table of ridge and toe with and without the extension and the stream discharge.  The columns come from
// examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/hillslope_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o hillslope_demo
//   ./hillslope_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

namespace {
constexpr int64_t N = 5;
elmk_ctx* site(bool hillslope)
{
  elmk_ctx* ctx = nullptr;
  chk(ctx, elmk_create(N, 0, &ctx), "elmk_create");
  chk(ctx, elmk_set_land(ctx, 1 /* soil */, 1, 12, 0, 0), "elmk_set_land");
  loam_columns(ctx, N, 0.6);
  put(ctx, "qflx_top_soil", N, std::vector<double>(1, 1.0e-4));  // rain that all reaches the soil, mm/s
  hydrology_on(ctx, N, 5.0e-3, 0.3, 0.05, 1.0e-4);
  hydrology_start(ctx, N, 2.0);
  if (hillslope) {
    std::vector<int32_t> down(N);
    std::vector<double> dist(N, 50.0), width(N, 30.0), area(N, 1500.0), elev(N);
    for (int64_t c = 0; c < N; c++) {
      down[c] = (int32_t)c - 1;  // column 0: -1, the stream
      elev[c] = 3.0 + 3.0 * (double)c;
    }
    chk(ctx, elmk_hillslope_enable(ctx, down.data(), dist.data(), width.data(), area.data(), elev.data(), 50.0), "elmk_hillslope_enable");
  }
  return ctx;
}
}  // namespace

int main()
{
  try {
    const double dt = 1800.0;
    const int nsteps = 96;
    elmk_ctx* on = site(true);
    elmk_ctx* off = site(false);
    std::printf("hillslope lateral flow, %d steps of %.0f s, %lld columns, toe = column 0\n", nsteps, dt, (long long)N);
    std::printf("%4s %12s %12s %14s %12s %12s\n", "step", "ZWT ridge m", "ZWT toe m", "QSTREAM m3/s", "ridge, off", "toe, off");
    std::vector<double> zon(N), zoff(N);
    double q = 0.0;
    bool ok = true;
    for (int s = 0; s < nsteps; s++) {
      chk(on, elmk_soil_hydrology(on, dt), "elmk_soil_hydrology");
      chk(off, elmk_soil_hydrology(off, dt), "elmk_soil_hydrology");
      chk(on, elmk_soil_hydrology_read(on, ELMK_HYD_ZWT, zon.data(), 0, N), "read");
      chk(off, elmk_soil_hydrology_read(off, ELMK_HYD_ZWT, zoff.data(), 0, N), "read");
      chk(on, elmk_hillslope_budget(on, &q), "elmk_hillslope_budget");
      std::printf("%4d %12.6f %12.6f %14.6e %12.6f %12.6f\n", s, zon[N - 1], zon[0], q, zoff[N - 1], zoff[0]);
      ok = ok && std::isfinite(zon[0]) && std::isfinite(zon[N - 1]) && std::isfinite(q) && q > 0.0;
    }
    ok = ok && zon[0] < zon[N - 1] && zoff[0] == zoff[N - 1];
    chk(on, elmk_destroy(on), "elmk_destroy");
    chk(off, elmk_destroy(off), "elmk_destroy");
    return ok ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hillslope_demo: %s\n", e.what());
    return 1;
  }
}
