/* elmk_solar.h - the solar lines of kokkos_init_timestep (init_timestep_kokkos.cc:26-34) for every column of a context:
 * the step-averaged cosine of the solar zenith angle (incident_shortwave.cc:14-121), the day length of the column and its
 * yearly maximum (day_length.cc:15-39), and canopy_fluxes' day-length factor (photosynthesis_impl.hh:28-44).
 *
 * The work is split by what varies, and every value keeps the reference's operation order (the build uses -ffp-contract=off):
 *   - per column, time-invariant (elmk_set_column_geography, host libm, so the reference's bits by construction):
 *     elmk_solar_column_consts -> one row of ELMK_GEO_N doubles;
 *   - per step, one value for all columns (elmk_solar_geometry, host libm): elmk_solar_step_consts;
 *   - per step and column: elmk_solar_column, on the device (k_solar.hip) with elmk_sin / elmk_acos, the restatements of
 *     the host libm's own algorithms.
 * The header compiles for the host as well (tests/c/solar_columns.cc pins the composition against the reference).
 *
 * Where the reference takes the sine and the cosine of one angle (integrate_cosz's latrad and declin, daylength's my_lat and
 * decl), its build calls glibc's sincos() once for both, and sincos is not bit for bit sin and cos (about one argument in
 * 1500 differs in the last bit).  The host part here calls sincos at the same places, explicitly, whatever the compiler
 * would have merged. */
#pragma once
#include "elmk_math.h"

/* rows of the per-column constants */
enum {
  ELMK_GEO_LON = 0,    /* lon_r */
  ELMK_GEO_TAN_LAT,    /* tan(ensure_tan_defined(lat_r))  (coshalfday, incident_shortwave.cc:54) */
  ELMK_GEO_SIN_LAT,    /* sin(lat_r), cos(lat_r)           (integrate_cosz, :105-106) */
  ELMK_GEO_COS_LAT,
  ELMK_GEO_SIN_MYLAT,  /* sin(my_lat), cos(my_lat)         (daylength, day_length.cc:28-29) */
  ELMK_GEO_COS_MYLAT,
  ELMK_GEO_MAX_DAYL,   /* max_daylength(lat_r)             (day_length.cc:39) */
  ELMK_GEO_N
};

/* the per-step scalars: the same for every column */
typedef struct {
  double s;                                  /* (decday - floor(decday)) * TWO_PI   (dt_start_rad, :38) */
  double dtrad;                              /* dt * TWO_PI / 86400                  (dt_radians, :34) */
  double tan_decl, sin_decl, cos_decl;       /* of declination_angle_sin((int)decday)  (average_cosz, :117) */
  double sin_decl_dl, cos_decl_dl;           /* of declination_angle_sin(doy + 1)      (init_timestep_kokkos.cc:33-34) */
} elmk_solar_step;

#define ELMK_SOLAR_PI 3.14159265358979323846 /* ELMconst::ELM_PI */
#define ELMK_SOLAR_TWO_PI (ELMK_SOLAR_PI * 2.0)

/* std::min / std::max of <algorithm>: the first argument wins ties and NaNs (host and device) */
#if defined(__HIPCC__)
#define ELMK_SOL_HD __host__ __device__ __forceinline__
#else
#define ELMK_SOL_HD static inline
#endif
ELMK_SOL_HD double elmk_sol_min(double a, double b) { return (b < a) ? b : a; }
ELMK_SOL_HD double elmk_sol_max(double a, double b) { return (a < b) ? b : a; }

/* ---- host part (in a HIP translation unit: host functions) ---- */
#include <math.h>

/* glibc's sincos (a GNU extension of <math.h>), declared here for C translation units without _GNU_SOURCE */
#if !defined(__cplusplus) && !defined(_GNU_SOURCE)
extern void sincos(double, double*, double*);
#endif

/* incident_shortwave.cc:17 */
static inline double elmk_solar_declination_angle_sin(int doy)
{
  return 23.45 * ELMK_SOLAR_PI / 180.0 * sin(ELMK_SOLAR_TWO_PI * (284.0 + doy) / 365.0);
}
/* :29-31 */
static inline double elmk_solar_ensure_tan_defined(double v)
{
  const double p2 = ELMK_SOLAR_PI / 2.0;
  return (v == p2) ? v - 1.0e-05 : (v == -p2) ? v + 1.0e-05 : v;
}
/* day_length.cc:20-28 */
static inline double elmk_solar_lat_epsilon(void) { return 10.0 * 2.220446049250313e-16; }
static inline double elmk_solar_my_lat(double lat)
{
  const double offset_pole = ELMK_SOLAR_PI / 2.0 - elmk_solar_lat_epsilon();
  return elmk_sol_min(offset_pole, elmk_sol_max(1.0 * offset_pole, lat));  /* (the reference's own expression) */
}
/* day_length.cc:15-34 */
static inline double elmk_solar_daylength_host(double lat, double decl)
{
  double sin_my, cos_my, sin_d, cos_d;
  sincos(elmk_solar_my_lat(lat), &sin_my, &cos_my);
  sincos(decl, &sin_d, &cos_d);
  double temp = -(sin_my * sin_d) / (cos_my * cos_d);
  temp = elmk_sol_min(1.0, elmk_sol_max(-1.0, temp));
  return 2.0 * 13750.9871 * acos(temp);
}
/* the range day_length.cc:22 asserts (|lat| <= pi/2 within 10 eps), finite longitude */
static inline int elmk_solar_geography_ok(double lat, double lon)
{
  return fabs(lat) <= ELMK_SOLAR_PI / 2.0 + elmk_solar_lat_epsilon() && isfinite(lon);
}
/* one column's time-invariant row (g[ELMK_GEO_N]) */
static inline void elmk_solar_column_consts(double lat, double lon, double* g)
{
  /* (the reference calls daylength out of line, so the declination constant is not folded at compile time: nor is it here) */
  volatile double max_decl = 0.409571;
  g[ELMK_GEO_LON] = lon;
  g[ELMK_GEO_TAN_LAT] = tan(elmk_solar_ensure_tan_defined(lat));
  sincos(lat, &g[ELMK_GEO_SIN_LAT], &g[ELMK_GEO_COS_LAT]);
  sincos(elmk_solar_my_lat(lat), &g[ELMK_GEO_SIN_MYLAT], &g[ELMK_GEO_COS_MYLAT]);
  g[ELMK_GEO_MAX_DAYL] = (lat < 0.0) ? elmk_solar_daylength_host(lat, -max_decl) : elmk_solar_daylength_host(lat, max_decl);
}
/* the step's scalars: decday = decimal_doy(date) + 1.0, doy = date.doy (init_timestep_kokkos.cc:29-34) */
static inline elmk_solar_step elmk_solar_step_consts(double dt, double decday, int doy)
{
  elmk_solar_step p;
  const double declin = elmk_solar_declination_angle_sin((int)decday);
  const double decl_dl = elmk_solar_declination_angle_sin(doy + 1);
  p.s = (decday - floor(decday)) * ELMK_SOLAR_TWO_PI;
  p.dtrad = dt * ELMK_SOLAR_TWO_PI / 86400.0;
  p.tan_decl = tan(elmk_solar_ensure_tan_defined(declin));
  sincos(declin, &p.sin_decl, &p.cos_decl);
  sincos(decl_dl, &p.sin_decl_dl, &p.cos_decl_dl);
  return p;
}

/* average_cosz (incident_shortwave.cc:114-121 with :37-94, :99-110) of one column from its row g and the step's scalars: the
 * cos(zenith) part of elmk_solar_column, on its own for the forcing interval's mean (elmk_set_forcing_record_time, k_solar.hip).
 * Reads g[ELMK_GEO_LON .. ELMK_GEO_COS_LAT] and p->s, dtrad, tan_decl, sin_decl, cos_decl. */
ELMK_MFN double elmk_solar_avg_cosz(const double g[ELMK_GEO_N], const elmk_solar_step* p)
{
  const double PI = ELMK_SOLAR_PI, TWO_PI = ELMK_SOLAR_TWO_PI;
  const double lon = g[ELMK_GEO_LON], tan_lat = g[ELMK_GEO_TAN_LAT];
  const double sin_lat = g[ELMK_GEO_SIN_LAT], cos_lat = g[ELMK_GEO_COS_LAT];
  const double dtrad = p->dtrad;
  // dt_start_rad / dt_end_rad (:37-48)
  double t_start = (p->s + lon) - PI;
  t_start = (t_start >= PI) ? t_start - TWO_PI : (t_start < -PI) ? t_start + TWO_PI : t_start;
  const double t_end = t_start + dtrad;
  // coshalfday (:52-56)
  const double ch = -tan_lat * p->tan_decl;
  const double cos_h = (ch <= -1.0) ? PI : (ch >= 1.0) ? 0.0 : elmk_acos(ch);
  // avg_hourangle (:61-94)
  double h0, h1, h2, h3;
  if (t_end >= PI && t_start <= PI && PI - cos_h <= dtrad) {
    h0 = elmk_sol_min(elmk_sol_max(t_start, -cos_h), cos_h);
    h1 = cos_h;
    h2 = TWO_PI - cos_h;
    h3 = elmk_sol_min(elmk_sol_max(t_end, TWO_PI - cos_h), TWO_PI + cos_h);
  } else if (t_end >= -PI && t_start <= -PI && PI - cos_h <= dtrad) {
    h0 = elmk_sol_min(elmk_sol_max(t_start, -TWO_PI - cos_h), -TWO_PI + cos_h);
    h1 = -TWO_PI + cos_h;
    h2 = -cos_h;
    h3 = elmk_sol_min(elmk_sol_max(t_end, -cos_h), cos_h);
  } else {
    const double a = (t_start > PI) ? t_start - TWO_PI : (t_start < -PI) ? t_start + TWO_PI : t_start;
    const double b = (t_end > PI) ? t_end - TWO_PI : (t_end < -PI) ? t_end + TWO_PI : t_end;
    h0 = elmk_sol_min(elmk_sol_max(a, -cos_h), cos_h);
    h1 = elmk_sol_min(elmk_sol_max(b, -cos_h), cos_h);
    h2 = 0.0;
    h3 = 0.0;
  }
  // integrate_cosz (:99-110)
  const double aa = sin_lat * p->sin_decl;
  const double bb = cos_lat * p->cos_decl;
  double cosz = 0.0;
  if (h1 > h0 || h3 > h2)
    cosz = (aa * (h1 - h0) + bb * (elmk_sin(h1) - elmk_sin(h0))) / dtrad + (aa * (h3 - h2) + bb * (elmk_sin(h3) - elmk_sin(h2))) / dtrad;
  return cosz;
}

/* The per-step, per-column part: average_cosz (elmk_solar_avg_cosz) and daylength (day_length.cc:29-33) from the column's row g
 * and the step's scalars; the day-length factor of canopy_fluxes (photosynthesis_impl.hh:33: min(1, max(0.01, dayl^2 / max_dayl^2))) */
ELMK_MFN void elmk_solar_column(const double g[ELMK_GEO_N], const elmk_solar_step* p, double* cosz_out, double* dayl_out,
                                double* dayl_factor_out)
{
  const double sin_my = g[ELMK_GEO_SIN_MYLAT], cos_my = g[ELMK_GEO_COS_MYLAT];
  const double mdl = g[ELMK_GEO_MAX_DAYL];
  const double cosz = elmk_solar_avg_cosz(g, p);
  // daylength (day_length.cc:29-33) of declination_angle_sin(doy + 1)
  double temp = -(sin_my * p->sin_decl_dl) / (cos_my * p->cos_decl_dl);
  temp = elmk_sol_min(1.0, elmk_sol_max(-1.0, temp));
  const double dl = 2.0 * 13750.9871 * elmk_acos(temp);
  *cosz_out = cosz;
  *dayl_out = dl;
  *dayl_factor_out = elmk_sol_min(1.0, elmk_sol_max(0.01, (dl * dl) / (mdl * mdl)));
}
