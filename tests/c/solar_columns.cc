// extern "C" view of the host build of elmkernels_amd/csrc/elmk_solar.h - the precompute elmk_set_column_geography /
// elmk_solar_geometry run on the host, then the per-column routine the device runs - for tests/test_solar_geometry_host.py.
// Build: g++ -O2 -mfma -ffp-contract=off -shared -fPIC (only the explicit fma() calls of elmk_math.h fuse, as on the device).
#include "elmk_solar.h"
extern "C" void elmk_test_solar_columns(long n, const double* lat, const double* lon, const double* dt, const double* decday,
                                        const int* doy, double* cosz, double* dayl, double* max_dayl, double* dayl_factor)
{
  for (long i = 0; i < n; i++) {
    double g[ELMK_GEO_N];
    elmk_solar_column_consts(lat[i], lon[i], g);
    const elmk_solar_step p = elmk_solar_step_consts(dt[i], decday[i], doy[i]);
    elmk_solar_column(g, &p, &cosz[i], &dayl[i], &dayl_factor[i]);
    max_dayl[i] = g[ELMK_GEO_MAX_DAYL];
  }
}
extern "C" int elmk_test_solar_geography_ok(double lat, double lon) { return elmk_solar_geography_ok(lat, lon); }
