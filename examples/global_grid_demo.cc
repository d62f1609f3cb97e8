// global_grid_demo.cc - per-column solar geometry for a grid that spans both hemispheres and every longitude, through
// include/elmk_interface.hpp: set the geography once, then kokkos_init_timestep's solar lines for every column at its own
// location, once per step, on the device.  Steps one simulated day (48 half-hour steps from midnight UTC of day 172) and prints,
// per step, the fraction of columns in daylight (step-averaged cos(zenith) > 0) and the day length of two columns.
//
//   g++ -std=c++17 -Iinclude examples/global_grid_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o demo
//   ./demo [ncols]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "elmk_interface.hpp"

int main(int argc, char** argv)
{
  const int64_t n = argc > 1 ? std::atoll(argv[1]) : 65536;
  if (n < 2) return 2;
  try {
    // a regular grid: rows of latitude from pole to pole (cell centres), columns of longitude around the globe
    const int64_t nlon = 64, nlat = (n + nlon - 1) / nlon;
    std::vector<double> lat(n), lon(n);
    for (int64_t c = 0; c < n; c++) {
      lat[c] = (-90.0 + 180.0 * ((double)(c / nlon) + 0.5) / (double)nlat) * M_PI / 180.0;
      lon[c] = (-180.0 + 360.0 * (double)(c % nlon) / (double)nlon) * M_PI / 180.0;
    }
    elmk::ELMInterface elm(n, 0);
    elm.set_column_geography(lat.data(), lon.data());
    const double dt = 1800.0;
    std::vector<double> cosz(n), dayl(n), max_dayl(n);
    for (int step = 0; step < 48; step++) {
      const double decday = 172.0 + step * dt / 86400.0;  // decimal_doy(date) + 1.0
      elm.solar_geometry(dt, decday, (int)decday - 1);
      elm.download("coszen", cosz.data());
      if (elmk_download_day_length(elm.context(), dayl.data(), max_dayl.data()) != ELMK_OK)
        throw std::runtime_error(elmk_last_error(elm.context()));
      int64_t day = 0;
      for (int64_t c = 0; c < n; c++) day += cosz[c] > 0.0;
      std::printf("step %2d  decday %.4f  day fraction %.4f  night fraction %.4f  dayl north %.1f s / south %.1f s\n", step, decday,
                  (double)day / (double)n, (double)(n - day) / (double)n, dayl[n - 1], dayl[0]);
    }
    elm.clear_column_geography();
  } catch (const std::exception& e) {
    std::fprintf(stderr, "global_grid_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
