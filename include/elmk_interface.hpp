/* elmk_interface.hpp - the C++ host side above the C ABI of elmk.h: a header-only mirror of the reference's driver class
 * ELM::ELMInterface (driver/kokkos/elm_kokkos_interface.hh:11-28, elm_kokkos_interface.cc:38-358) for a caller that links
 * libelmk instead of the reference's Kokkos wrappers.  Same member names, same call order in advance(), same PrimaryVars
 * members (src/data/elm_state.h:17-48).  What the reference's class also does - opening the NetCDF surface / forcing /
 * parameter files and the date arithmetic of kokkos_init_timestep - stays with the caller (control plane, out of scope:
 * DESIGN.md section 8): the caller uploads the bracketing forcing / phenology records and passes the interpolation weights.
 *
 *   elmk::ELMInterface elm(ncols, gpu);                    // was ELM::ELMInterface elm(ncols);
 *   elm.setup(land, pft_psn, pft_alb, ..., snicar, age);   // was elm.setup();  (the files' contents, read by the caller)
 *   elm.upload("t_soisno", host_ptr);  ...                 // was initialize_kokkos_elm(*S_, files ...)
 *   bool failed = elm.advance(dt_seconds, w);              // was elm.advance(dt_start_date, dt_seconds);
 *   auto pv = elm.getPrimaryVars();                        // same
 *
 * Nothing here touches HIP or torch: plain C++17 over the extern "C" entry points. */
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "elmk.h"

namespace elmk {

/* The host scalars kokkos_init_timestep computes before its kernels (init_timestep_kokkos.cc:26-34): the cosine of the solar
 * zenith angle averaged over the step, the day length and its yearly maximum.  Plain <cmath> on the host, as in the
 * reference (src/physics/incident_shortwave.cc:14-121, day_length.cc:15-39), so the values are the reference's bits on the
 * same libm; checked against the reference's own sources compiled into oracle/_ref (tests/test_host_side.py). */
namespace solar {
constexpr double PI = 3.14159265358979323846;  // ELMconst::ELM_PI
constexpr double TWO_PI = PI * 2.0;
constexpr double PI_OVER_TWO = PI / 2.0;

/* incident_shortwave.cc:17 (lnd_import szenith() / shr_orb_cosz()) */
inline double declination_angle_sin(int doy) { return 23.45 * PI / 180.0 * std::sin(TWO_PI * (284.0 + doy) / 365.0); }
/* :29-31 */
inline double ensure_tan_defined(double var) { return (var == PI_OVER_TWO) ? var - 1.0e-05 : (var == -PI_OVER_TWO) ? var + 1.0e-05 : var; }
/* :37-42: start of the step as an hour angle on [-pi, pi) */
inline double dt_start_rad(double jday, double lonrad)
{
  const double t_start = (jday - std::floor(jday)) * TWO_PI + lonrad - PI;
  return (t_start >= PI) ? t_start - TWO_PI : (t_start < -PI) ? t_start + TWO_PI : t_start;
}
/* :52-56: half-day length [0, pi] */
inline double coshalfday(double latrad, double declin)
{
  const double cos_h = -std::tan(ensure_tan_defined(latrad)) * std::tan(ensure_tan_defined(declin));
  return (cos_h <= -1.0) ? PI : (cos_h >= 1.0) ? 0.0 : std::acos(cos_h);
}
/* :61-94 */
inline void avg_hourangle(double t_start, double t_end, double dtrad, double cos_h, double ha[4])
{
  auto clamp = [](double v, double lo, double hi) { return std::min(std::max(v, lo), hi); };
  if (t_end >= PI && t_start <= PI && PI - cos_h <= dtrad) {
    ha[0] = clamp(t_start, -cos_h, cos_h);
    ha[1] = cos_h;
    ha[2] = TWO_PI - cos_h;
    ha[3] = clamp(t_end, TWO_PI - cos_h, TWO_PI + cos_h);
  } else if (t_end >= -PI && t_start <= -PI && PI - cos_h <= dtrad) {
    ha[0] = clamp(t_start, -TWO_PI - cos_h, -TWO_PI + cos_h);
    ha[1] = -TWO_PI + cos_h;
    ha[2] = -cos_h;
    ha[3] = clamp(t_end, -cos_h, cos_h);
  } else {
    ha[0] = clamp((t_start > PI) ? t_start - TWO_PI : (t_start < -PI) ? t_start + TWO_PI : t_start, -cos_h, cos_h);
    ha[1] = clamp((t_end > PI) ? t_end - TWO_PI : (t_end < -PI) ? t_end + TWO_PI : t_end, -cos_h, cos_h);
    ha[2] = 0.0;
    ha[3] = 0.0;
  }
}
/* :98-121: Zhou et al. (2015) average of cos(zenith) over [t, t + dt] */
inline double average_cosz(double latrad, double lonrad, double dt, double jday)
{
  const double dtrad = dt * TWO_PI / 86400.0;
  const double t_start = dt_start_rad(jday, lonrad);
  const double t_end = t_start + dtrad;
  const double declin = declination_angle_sin(static_cast<int>(jday));
  const double cos_h = coshalfday(latrad, declin);
  const double aa = std::sin(latrad) * std::sin(declin);
  const double bb = std::cos(latrad) * std::cos(declin);
  double ha[4];
  avg_hourangle(t_start, t_end, dtrad, cos_h, ha);
  return (ha[1] > ha[0] || ha[3] > ha[2])
             ? (aa * (ha[1] - ha[0]) + bb * (std::sin(ha[1]) - std::sin(ha[0]))) / dtrad +
                   (aa * (ha[3] - ha[2]) + bb * (std::sin(ha[3]) - std::sin(ha[2]))) / dtrad
             : 0.0;
}
/* day_length.cc:15-34 (seconds); lat and decl in radians */
inline double daylength(double lat, double decl)
{
  const double secs_per_radian = 13750.9871;
  const double lat_epsilon = 10.0 * 2.220446049250313e-16;
  const double offset_pole = PI / 2.0 - lat_epsilon;
  const double my_lat = std::min(offset_pole, std::max(1.0 * offset_pole, lat));  // (the reference's own expression, :28)
  double temp = -(std::sin(my_lat) * std::sin(decl)) / (std::cos(my_lat) * std::cos(decl));
  temp = std::min(1.0, std::max(-1.0, temp));
  return 2.0 * secs_per_radian * std::acos(temp);
}
/* :39 */
inline double max_daylength(double lat) { return (lat < 0.0) ? daylength(lat, -0.409571) : daylength(lat, 0.409571); }
}  // namespace solar

/* ELM::PrimaryVars<ViewI1, ViewD1, ViewD2> (src/data/elm_state.h:17-48) on the host: [column][level], level fastest,
 * as the reference's Views are (src/utils/array.hh:176-179) */
struct PrimaryVars {
  explicit PrimaryVars(int64_t ncols)
      : snl(ncols), nrad(ncols), snow_depth(ncols), frac_sno(ncols), int_snow(ncols), h2ocan(ncols), h2osno(ncols),
        h2osfc(ncols), t_grnd(ncols), t_h2osfc(ncols), t_h2osfc_bef(ncols), snw_rds(ncols * 5), h2osoi_liq(ncols * 20),
        h2osoi_ice(ncols * 20), h2osoi_vol(ncols * 15), t_soisno(ncols * 20), dz(ncols * 20), zsoi(ncols * 20),
        zisoi(ncols * 21)
  {
  }
  std::vector<int32_t> snl, nrad;
  std::vector<double> snow_depth, frac_sno, int_snow, h2ocan, h2osno, h2osfc, t_grnd, t_h2osfc, t_h2osfc_bef;
  std::vector<double> snw_rds, h2osoi_liq, h2osoi_ice, h2osoi_vol, t_soisno, dz, zsoi, zisoi;
};

/* what kokkos_init_timestep's host part yields per step (init_timestep_kokkos.cc:17-52): the interpolation weights of
 * the two bracketing forcing records and of the two bracketing months; the records themselves are uploaded by the caller
 * (fields atm_* and mlai .. mhbot, ELMK_LAYOUT_SOA) whenever the bracket moves */
struct StepWeights {
  double forc_wt1[8], forc_wt2[8];  // per stream: TBOT, PBOT, QBOT|RH, FLDS, FSDS, PREC, WIND, ZBOT (atm_data_impl.hh:191-199)
  double month_wt1, month_wt2;
  int qbot_is_relative_humidity;
};

class ELMInterface {
 public:
  ELMInterface(int64_t ncols, int gpu = 0) : ncols_(ncols)
  {
    if (elmk_create(ncols, gpu, &ctx_) != ELMK_OK) throw std::runtime_error(elmk_last_error(nullptr));
  }
  ~ELMInterface() { (void)elmk_destroy(ctx_); }
  ELMInterface(const ELMInterface&) = delete;
  ELMInterface& operator=(const ELMInterface&) = delete;

  /* ELMInterface::setup (elm_kokkos_interface.cc:58-267) minus the file reads: parameters that the reference's state
   * object carries beside its Views */
  void setup(int ltype, int ctype, int vtype, int urbpoi, int lakpoi, double dewmx, int oldfflag, double dayl, double max_dayl,
             const double* pft_psn, const double* pft_alb, const double* z0mr, const double* displar, const double* albsat,
             const double* albdry, const elmk_snicar_tables* snicar, const double* age_tau, const double* age_kappa,
             const double* age_drdt0)
  {
    ok(elmk_set_land(ctx_, ltype, ctype, vtype, urbpoi, lakpoi));
    ok(elmk_set_scalars(ctx_, dewmx, oldfflag, dayl, max_dayl));
    ok(elmk_set_pft(ctx_, pft_psn, pft_alb, z0mr, displar));
    ok(elmk_set_soilcolor(ctx_, albsat, albdry));
    ok(elmk_set_snicar(ctx_, snicar));
    ok(elmk_set_snow_age_tables(ctx_, age_tau, age_kappa, age_drdt0));
    ok(elmk_set_graph(ctx_, 1));  // advance() replays one HIP graph per step
  }

  /* the per-column part of ELM::initialize_kokkos_elm (initialize_elm_kokkos.cc:373-428): cold-start state from the
   * uploaded topography, snow depth, soil texture (fields pct_sand, pct_clay, organic) and PFT; call after the uploads */
  void initialize(double organic_max, const double* roota_par, const double* rootb_par)
  {
    ok(elmk_set_init_params(ctx_, organic_max, roota_par, rootb_par));
    ok(elmk_initialize_state(ctx_));
  }

  /* one ELMStateViews member, host layout of the reference ([column][level]) */
  void upload(const char* field, const void* host) { ok(elmk_upload(ctx_, id(field), host, 0, ncols_, ELMK_LAYOUT_COL_MAJOR)); }
  void download(const char* field, void* host) { ok(elmk_download(ctx_, id(field), host, 0, ncols_, ELMK_LAYOUT_COL_MAJOR)); }

  /* ELMInterface::advance (elm_kokkos_interface.cc:269-322): kokkos_init_timestep's per-column work, then the ten physics
   * calls in the reference's order, then kokkos_evaluate_conservation.  Returns false like the reference ("failed"
   * flag); a raised throw / assert site of the reference's physics becomes one exception per step. */
  bool advance(double dt_seconds, const StepWeights& w)
  {
    ok(elmk_phenology(ctx_, w.month_wt1, w.month_wt2));
    ok(elmk_get_forcing(ctx_, w.forc_wt1, w.forc_wt2, w.qbot_is_relative_humidity));
    ok(elmk_init_timestep(ctx_));
    if (irrigation_) {  // the split form of elmk_advance_physics with the irrigation stage in it (elmk.h "irrigation")
      ok(elmk_timestep7_fused(ctx_, dt_seconds));
      ok(elmk_irrigation(ctx_, dt_seconds, tod_));
      ok(elmk_soil_temperature(ctx_, dt_seconds));
      ok(elmk_snow_hydrology(ctx_, dt_seconds));
      ok(elmk_surface_fluxes(ctx_, dt_seconds));
    } else {
      ok(elmk_advance_physics(ctx_, dt_seconds));
    }
    ok(elmk_evaluate_conservation(ctx_, dt_seconds, &conservation_[0][0], nullptr));
    uint32_t flags = 0;
    int64_t col = -1;
    ok(elmk_error_summary(ctx_, &flags, &col));
    if (flags & ELMK_ERR_FATAL_MASK)
      throw std::runtime_error("ELM physics error flags " + std::to_string(flags) + ", first at column " + std::to_string(col));
    last_flags_ = flags;
    return false;
  }

  /* the host scalars of kokkos_init_timestep (init_timestep_kokkos.cc:26-34) for one location: coszen for every column
   * (Utils::assign(S.coszen, cosz)), S.dayl and S.max_dayl.  decday = Utils::decimal_doy(date) + 1.0, doy = date.doy. */
  void set_solar_geometry(double lat_r, double lon_r, double dt_seconds, double decday, int doy, double dewmx, int oldfflag)
  {
    ok(elmk_fill(ctx_, id("coszen"), solar::average_cosz(lat_r, lon_r, dt_seconds, decday)));
    ok(elmk_set_scalars(ctx_, dewmx, oldfflag, solar::daylength(lat_r, solar::declination_angle_sin(doy + 1)),
                        solar::max_daylength(lat_r)));
  }

  /* A domain whose columns do not share one sun (a regional or global grid): the latitude and longitude of every column, radians
   * ([ncols] each), once.  From then on solar_geometry() - or the advance() overload below - does kokkos_init_timestep's solar
   * lines for each column at its own location, on the device, and canopy_fluxes takes each column's own day length.
   * clear_column_geography() goes back to set_solar_geometry's single location. */
  void set_column_geography(const double* lat_r, const double* lon_r) { ok(elmk_set_column_geography(ctx_, lat_r, lon_r)); }
  void solar_geometry(double dt_seconds, double decday, int doy) { ok(elmk_solar_geometry(ctx_, dt_seconds, decday, doy)); }
  void clear_column_geography() { ok(elmk_clear_column_geography(ctx_)); }
  /* advance() for a grid with a geography: the solar lines first, then phenology and forcing (coszen feeds get_forcing's
   * direct / diffuse split, atm_physics_impl.hh), in kokkos_init_timestep's order (init_timestep_kokkos.cc:26-50).
   * decday = Utils::decimal_doy(date) + 1.0, doy = date.doy of the step's start. */
  bool advance(double dt_seconds, const StepWeights& w, double decday, int doy)
  {
    set_time_of_day(time_of_day(decday, doy));
    solar_geometry(dt_seconds, decday, doy);
    return advance(dt_seconds, w);
  }

  /* Shortwave (elmk_set_shortwave_mode): ELMK_SW_COSZEN spreads interval-mean FSDS records (forc_dt seconds each) over the steps of
   * their interval with ELM's cos(zenith) factor; needs the column geography.  The record start of each record, as decimal_doy + 1.0:
   * set_forcing_record_time() before a stepwise advance() for the record in level 0 of atm_*, series_record_times() for the forcing
   * slots of a run. */
  void set_shortwave_mode(int mode, double forc_dt_seconds) { ok(elmk_set_shortwave_mode(ctx_, mode, forc_dt_seconds)); }
  void set_forcing_record_time(double rec_decday) { ok(elmk_set_forcing_record_time(ctx_, rec_decday)); }
  void series_record_times(int slot0, int nslots, const double* rec_decday) { ok(elmk_series_record_times(ctx_, slot0, nslots, rec_decday)); }

  /* Downscaling (elmk_set_downscaling): ELMK_DS_TOPO adjusts every step's forcing from the forcing's surface height to each column's
   * elevation (lapse-rate temperature, hydrostatic pressure, kept relative humidity, longwave, rain / snow split).  The elevations
   * first: set_column_elevation() with both arrays, or with topo_forc = nullptr and then set_forcing_elevation_gridded() over the
   * forcing grid.  Optional longwave groups (CSR by gridcell) keep each gridcell's weighted mean longwave. */
  void set_column_elevation(const double* topo_col, const double* topo_forc) { ok(elmk_set_column_elevation(ctx_, topo_col, topo_forc)); }
  void set_forcing_elevation_gridded(const double* cells) { ok(elmk_set_forcing_elevation_gridded(ctx_, cells)); }
  void set_downscaling(int mode, double lapse = 0.006, double lapse_lw = 0.032, double lw_limit = 0.5)
  {
    ok(elmk_set_downscaling(ctx_, mode, lapse, lapse_lw, lw_limit));
  }
  void set_downscaling_groups(int64_t ngroups, const int64_t* ptr, const int32_t* col, const double* w)
  {
    ok(elmk_set_downscaling_groups(ctx_, ngroups, ptr, col, w));
  }
  void clear_downscaling_groups() { ok(elmk_clear_downscaling_groups(ctx_)); }

  /* History tapes (ELM's time-averaged output) kept on the device: register fields once, call accumulate_history() after every
   * advance(), read at the end of an output interval and reset the tape.  op: ELMK_HIST_AVG / _SUM / _MAX / _MIN / _INST;
   * history_add returns the entry id history_read takes.  history_read fills [ncols][nlev] doubles, the host layout of upload. */
  int history_add(int tape, const char* field, int op)
  {
    const int e = elmk_history_add(ctx_, tape, id(field), op);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  void accumulate_history() { ok(elmk_history_accumulate(ctx_)); }
  void history_reset(int tape) { ok(elmk_history_reset(ctx_, tape)); }
  int64_t history_count(int tape)
  {
    int64_t n = 0;
    ok(elmk_history_count(ctx_, tape, &n));
    return n;
  }
  void history_read(int entry, double* host) { ok(elmk_history_read(ctx_, entry, host, 0, ncols_, ELMK_LAYOUT_COL_MAJOR)); }
  void history_clear() { ok(elmk_history_clear(ctx_)); }

  /* Accumulated fields (elmk.h "accumulated fields"; ELM's accumulMod): accum_add() registers a running mean / period average /
   * running accumulation of `src` over period_steps steps, written to `dst` (nullptr: no destination) - accum_add_t10() is ELM's T10,
   * the 10-day running mean of t_ref2m into t10, which photosynthesis reads.  update_accum() after every advance() and before
   * accumulate_history(), or run(..., update_accum = true).  accum_init() sets the value ([nlev][ncols], SoA; nullptr: seeded from the
   * destination field) and the step count, as from a restart file; accum_read() fills [nlev][ncols] and returns the count. */
  int accum_add(const char* src, int kind, int64_t period_steps, const char* dst = nullptr)
  {
    const int e = elmk_accum_add(ctx_, id(src), kind, period_steps, dst ? id(dst) : -1);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  int accum_add_t10(double dt_seconds, int days = 10)
  {
    const double steps = days * 86400.0 / dt_seconds;
    if (!(steps >= 1.0) || steps != std::floor(steps)) throw std::invalid_argument("accum_add_t10: the period is not a whole number of steps");
    return accum_add("t_ref2m", ELMK_ACCUM_RUNMEAN, (int64_t)steps, "t10");
  }
  void accum_init(int entry, const double* host = nullptr, int64_t nsteps = 0) { ok(elmk_accum_init(ctx_, entry, host, nsteps)); }
  void update_accum() { ok(elmk_accum_update(ctx_)); }
  int64_t accum_read(int entry, double* host)
  {
    int64_t n = 0;
    ok(elmk_accum_read(ctx_, entry, host, 0, host ? ncols_ : 0, ELMK_LAYOUT_SOA, &n));
    return n;
  }
  void accum_clear() { ok(elmk_accum_clear(ctx_)); }

  /* Active layer thickness (elmk.h "active layer thickness"; ELM's ActiveLayerMod::alt_calc): active_layer_enable() allocates the rows
   * alt, altmax and altmax_lastyear; update_active_layer() after every advance() and before update_accum() computes the thaw depth from
   * t_soisno and keeps altmax_indx / altmax_lastyear_indx (0-based soil layers, -1: none) live, or run(..., update_active_layer = true)
   * does it in every step with the annual rollover on the steps that start at 00:00 of 1 January / 1 July.  active_layer_init() takes a
   * restart file's ALTMAX and ALTMAX_LASTYEAR ([ncols] each, nullptr: zeros); active_layer_read() fills [ncols] of row ELMK_ALT_*. */
  void active_layer_enable() { ok(elmk_active_layer_enable(ctx_)); }
  void active_layer_init(const double* altmax = nullptr, const double* altmax_lastyear = nullptr)
  {
    ok(elmk_active_layer_init(ctx_, altmax, altmax_lastyear));
  }
  void update_active_layer(int rollover = 0) { ok(elmk_active_layer_update(ctx_, rollover)); }
  void active_layer_read(int which, double* host) { ok(elmk_active_layer_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void active_layer_clear() { ok(elmk_active_layer_clear(ctx_)); }

  /* Soil hydrology (elmk.h "soil hydrology"; ELM v1's column hydrology, which the reference leaves to an external model):
   * soil_hydrology_enable() allocates the rows, soil_hydrology_set_params() takes hksat [10][ncols] and four [ncols] rows,
   * soil_hydrology_init() the water table and the aquifer (nullptr: ELM's cold start); soil_hydrology(dt) after every advance() applies
   * runoff, infiltration, the Richards solve, the water table and drainage, or run(..., soil_hydrology = true) does it in every step
   * before the conservation row.  soil_hydrology_read() fills [ncols] of row ELMK_HYD_*. */
  void soil_hydrology_enable() { ok(elmk_soil_hydrology_enable(ctx_)); }
  void soil_hydrology_set_params(const double* hksat, const double* wtfact, const double* h2osfc_thresh, const double* k_wet,
                                 const double* rsub_top_max)
  {
    ok(elmk_soil_hydrology_set_params(ctx_, hksat, wtfact, h2osfc_thresh, k_wet, rsub_top_max));
  }
  void soil_hydrology_init(const double* zwt = nullptr, const double* wa = nullptr) { ok(elmk_soil_hydrology_init(ctx_, zwt, wa)); }
  void soil_hydrology(double dt_seconds) { ok(elmk_soil_hydrology(ctx_, dt_seconds)); }
  void soil_hydrology_read(int which, double* host) { ok(elmk_soil_hydrology_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void soil_hydrology_clear() { ok(elmk_soil_hydrology_clear(ctx_)); }
  /* Irrigation (elmk.h "irrigation"; ELM's demand check and daily application): irrigation_enable(sched[ncols]) allocates the rows RATE,
   * NLEFT and QFLX_IRRIG and takes the schedule (-1: not irrigated, else the longitude offset in seconds 0 .. 86399); from then on
   * advance() takes the split form of the physics with the stage between the seven wrappers and soil_temperature, at the time of day
   * the advance() overload with decday / doy derives, or set_time_of_day() sets (seconds after midnight UTC at the step's start), and
   * run(..., irrigation = true) does the same in every step.  irrigation_init() takes a restart file's irrig_rate and
   * n_irrig_steps_left ([ncols] each, nullptr: zeros); irrigation_read() fills [ncols] of row ELMK_IRR_*. */
  void irrigation_enable(const int32_t* sched)
  {
    ok(elmk_irrigation_enable(ctx_, sched));
    irrigation_ = true;
  }
  void irrigation_init(const double* rate = nullptr, const double* nleft = nullptr) { ok(elmk_irrigation_init(ctx_, rate, nleft)); }
  void irrigation_read(int which, double* host) { ok(elmk_irrigation_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void irrigation_clear()
  {
    ok(elmk_irrigation_clear(ctx_));
    irrigation_ = false;
  }
  /* The river supply limit (elmk.h "irrigation: river supply limit"): irrigation_supply_enable(threshold) after irrigation_enable,
   * routing_enable and routing_set_withdrawal(true), with an output grid in which every column lies in at most one cell; from then
   * on every demand check - in advance() and in run(..., irrigation = true) - is cut back to what the cell's channel held at the end
   * of the previous step.  irrigation_supply_read() fills [ncells] of row ELMK_IRRSUP_*; irrigation_supply_init() takes a restart's
   * UNMET_SUM ([ncells], nullptr: zeros); irrigation_supply_reset() zeroes it; irrigation_supply_clear() switches the limit off. */
  void irrigation_supply_enable(double threshold = 0.1) { ok(elmk_irrigation_supply_enable(ctx_, threshold)); }
  void irrigation_supply_init(const double* unmet_sum = nullptr) { ok(elmk_irrigation_supply_init(ctx_, unmet_sum)); }
  void irrigation_supply_read(int which, double* host) { ok(elmk_irrigation_supply_read(ctx_, which, host, 0, host ? routing_ncells_ : 0)); }
  void irrigation_supply_reset() { ok(elmk_irrigation_supply_reset(ctx_)); }
  void irrigation_supply_clear() { ok(elmk_irrigation_supply_clear(ctx_)); }
  void set_time_of_day(int tod_seconds) { tod_ = tod_seconds; }
  /* llround((decday - 1.0 - doy) * 86400.0) reduced to 0 .. 86399, as elmk_run derives it */
  static int time_of_day(double decday, int doy)
  {
    const long long t = std::llround((decday - 1.0 - (double)doy) * 86400.0);
    return (int)(((t % 86400) + 86400) % 86400);
  }
  /* Its frost-table extension (elmk.h "soil hydrology", F'): from soil_hydrology_frost_enable(q_perch_max[ncols]) on the stage drains
   * perched water above a frozen layer; soil_hydrology_frost_read() fills [ncols] of row ELMK_HYDF_*. */
  void soil_hydrology_frost_enable(const double* q_perch_max) { ok(elmk_soil_hydrology_frost_enable(ctx_, q_perch_max)); }
  void soil_hydrology_frost_read(int which, double* host) { ok(elmk_soil_hydrology_frost_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void soil_hydrology_frost_clear() { ok(elmk_soil_hydrology_frost_clear(ctx_)); }
  /* Its hillslope lateral flow (elmk.h "hillslope lateral flow", L1 - L3): from hillslope_enable(down, dist, width, area, elev [ncols]
   * each, k_aniso) on the stage passes groundwater downhill along down[] (-1: the stream, -2: on no hillslope) and the lowest column
   * discharges to the stream; hillslope_read() fills [ncols] of row ELMK_HS_*, hillslope_budget() sums[1] with the stream discharge
   * (m3/s); hillslope_clear() returns to every column's own baseflow.  It excludes the frost table and the floodplain infiltration. */
  void hillslope_enable(const int32_t* down, const double* dist, const double* width, const double* area, const double* elev, double k_aniso)
  {
    ok(elmk_hillslope_enable(ctx_, down, dist, width, area, elev, k_aniso));
  }
  void hillslope_read(int which, double* host) { ok(elmk_hillslope_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void hillslope_rows(double* host /*[ELMK_HS_NROWS][ncols]*/)
  {
    for (int w = 0; w < ELMK_HS_NROWS; w++) hillslope_read(w, host + (size_t)w * (size_t)ncols_);
  }
  void hillslope_budget(double* sums) { ok(elmk_hillslope_budget(ctx_, sums)); }
  void hillslope_clear() { ok(elmk_hillslope_clear(ctx_)); }

  /* Water balance (elmk.h "water balance"): the closed column water budget of a step that runs the soil hydrology, with total runoff
   * QRUNOFF, total water storage ENDWB (ELM's TWS) and the soil-water rows.  water_balance_enable(tol_mm) allocates the rows;
   * water_balance_begin() after init_timestep and before the physics, water_balance(dt, ...) after soil_hydrology(dt) - it fills the
   * (min, max, sum) triples of ERRH2O, QRUNOFF, ENDWB ([3][3]), the number of columns with !(|ERRH2O| <= tol) and the first of them (any
   * pointer may be nullptr; all nullptr: no synchronisation) - or run(..., water_balance = true) does both in every step, after which
   * run_water_balance() fills [nsteps][3][3], [nsteps] and [nsteps] and returns nsteps.  water_balance_read() fills [ncols] of row ELMK_WB_*. */
  void water_balance_enable(double tol_mm) { ok(elmk_water_balance_enable(ctx_, tol_mm)); }
  void water_balance_begin() { ok(elmk_water_balance_begin(ctx_)); }
  void water_balance(double dt_seconds, double* min_max_sum = nullptr, int64_t* nbad = nullptr, int64_t* first_bad_col = nullptr)
  {
    ok(elmk_water_balance(ctx_, dt_seconds, min_max_sum, nbad, first_bad_col));
  }
  void water_balance_read(int which, double* host) { ok(elmk_water_balance_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void water_balance_clear() { ok(elmk_water_balance_clear(ctx_)); }
  int run_water_balance(double* min_max_sum, int64_t* nbad, int64_t* first_bad_col)
  {
    const int n = elmk_run_water_balance(ctx_, min_max_sum, nbad, first_bad_col);
    ok(n < 0 ? n : ELMK_OK);
    return n;
  }
  /* Runoff routing (elmk.h "runoff routing"): the linear-reservoir river model over the output grid's cells.  routing_enable() takes the
   * network (down[ncells], -1 = an outlet; ddist metres; area square metres) after set_output_grid and water_balance_enable;
   * routing(dt) after water_balance(dt), or run(..., routing = true) in every step.  routing_read() fills [ncells] of row ELMK_ROUTE_*;
   * routing_init() takes a restart's VOLR, QOUT_SUM ([ncells] each, nullptr: zeros) and call count; routing_budget() fills sums[3]. */
  void routing_enable(int64_t ncells, const int32_t* down, const double* ddist, const double* area, double effvel = 0.35, int nsub = 1)
  {
    ok(elmk_routing_enable(ctx_, ncells, down, ddist, area, effvel, nsub));
    routing_ncells_ = ncells;
  }
  void routing_init(const double* volr = nullptr, const double* qout_sum = nullptr, int64_t ncalls = 0)
  {
    ok(elmk_routing_init(ctx_, volr, qout_sum, ncalls));
  }
  void routing(double dt_seconds) { ok(elmk_routing(ctx_, dt_seconds)); }
  void routing_read(int which, double* host) { ok(elmk_routing_read(ctx_, which, host, 0, host ? routing_ncells_ : 0)); }
  int64_t routing_count()
  {
    int64_t n = 0;
    ok(elmk_routing_count(ctx_, &n));
    return n;
  }
  void routing_reset_mean() { ok(elmk_routing_reset_mean(ctx_)); }
  void routing_set_withdrawal(bool on) { ok(elmk_routing_set_withdrawal(ctx_, on ? 1 : 0)); }
  void routing_budget(double* sums) { ok(elmk_routing_budget(ctx_, sums)); }
  void routing_clear() { ok(elmk_routing_clear(ctx_)); }
  /* Kinematic-wave routing (elmk.h "kinematic-wave routing"): the routing stage's second scheme, through hillslope, tributaries and
   * main channel.  routing_kinematic_enable() takes params[ELMK_KW_NPARAM][ncells] after routing_enable and soil_hydrology_enable;
   * routing(dt) and run(..., routing = true) then run it, and routing_read() takes ELMK_ROUTE_WH, ELMK_ROUTE_WT and ELMK_ROUTE_QSUR as
   * well.  routing_kinematic_init() takes a restart's WH and WT ([ncells] each, nullptr: zeros); routing_kinematic_budget() fills
   * sums[2]; routing_kinematic_clear() returns to the linear scheme and keeps VOLR, QOUT_SUM and the count. */
  void routing_kinematic_enable(const double* params) { ok(elmk_routing_kinematic_enable(ctx_, params)); }
  void routing_kinematic_init(const double* wh = nullptr, const double* wt = nullptr) { ok(elmk_routing_kinematic_init(ctx_, wh, wt)); }
  void routing_kinematic_budget(double* sums) { ok(elmk_routing_kinematic_budget(ctx_, sums)); }
  void routing_kinematic_clear() { ok(elmk_routing_kinematic_clear(ctx_)); }
  /* Floodplain inundation (elmk.h "floodplain inundation"): banks and a floodplain for the kinematic scheme's main channel.
   * routing_inundation_enable() takes rdepth[ncells] and eprof[ELMK_FP_NPROF][ncells] after routing_kinematic_enable; routing(dt) and
   * run(..., routing = true) then run the flood form, and routing_read() takes ELMK_ROUTE_WF, ELMK_ROUTE_FLOOD_DEPTH and
   * ELMK_ROUTE_FLOOD_FRAC as well.  routing_inundation_init() takes a restart's WF ([ncells], nullptr: zeros);
   * routing_inundation_budget() fills sums[1]; routing_inundation_clear() returns to the channel without banks and keeps VOLR. */
  void routing_inundation_enable(const double* rdepth, const double* eprof) { ok(elmk_routing_inundation_enable(ctx_, rdepth, eprof)); }
  void routing_inundation_init(const double* wf = nullptr) { ok(elmk_routing_inundation_init(ctx_, wf)); }
  void routing_inundation_budget(double* sums) { ok(elmk_routing_inundation_budget(ctx_, sums)); }
  void routing_inundation_clear() { ok(elmk_routing_inundation_clear(ctx_)); }
  /* Reservoirs (elmk.h "reservoirs"): dams at the outlets of the kinematic scheme's cells.  routing_reservoir_enable() takes cap[ncells]
   * (0 = no dam), target[12][ncells], beta[ncells] and mstart[ncells] after routing_kinematic_enable; routing(dt) and
   * run(..., routing = true) then run the DAM form, and routing_read() takes ELMK_ROUTE_RES, ELMK_ROUTE_KRLS and ELMK_ROUTE_RES_TAKE as
   * well.  routing_reservoir_time() sets the month and `begins` of the following routing(dt) calls (run() takes them from its steps);
   * routing_reservoir_init() takes a restart's RES and KRLS ([ncells], nullptr: zeros and 1.0); routing_reservoir_budget() fills
   * sums[2]; routing_reservoir_clear() returns to the free-flowing channel and keeps VOLR. */
  void routing_reservoir_enable(const double* cap, const double* target, const double* beta, const int32_t* mstart)
  {
    ok(elmk_routing_reservoir_enable(ctx_, cap, target, beta, mstart));
  }
  void routing_reservoir_init(const double* res = nullptr, const double* krls = nullptr) { ok(elmk_routing_reservoir_init(ctx_, res, krls)); }
  void routing_reservoir_time(int month, bool begins) { ok(elmk_routing_reservoir_time(ctx_, month, begins ? 1 : 0)); }
  void routing_reservoir_budget(double* sums) { ok(elmk_routing_reservoir_budget(ctx_, sums)); }
  void routing_reservoir_clear() { ok(elmk_routing_reservoir_clear(ctx_)); }
  /* Stream temperature (elmk.h "stream temperature"): the tributary store and the main channel of the kinematic scheme's cells carry a
   * temperature.  routing_heat_enable() takes the soil layer of the subsurface runoff's temperature and shade[ncells] (nullptr: 0) after
   * routing_kinematic_enable, without the inundation and the reservoirs; routing(dt) and run(..., routing = true) then run the HEAT
   * form, and routing_read() takes ELMK_ROUTE_TT .. ELMK_ROUTE_HOUT as well.  routing_heat_init() takes a restart's TT and TR
   * ([ncells], nullptr: 273.15 K); routing_heat_budget() fills sums[5]; routing_heat_clear() drops the temperatures and keeps the water. */
  void routing_heat_enable(int sublev = 0, const double* shade = nullptr) { ok(elmk_routing_heat_enable(ctx_, sublev, shade)); }
  void routing_heat_init(const double* tt = nullptr, const double* tr = nullptr) { ok(elmk_routing_heat_init(ctx_, tt, tr)); }
  void routing_heat_budget(double* sums) { ok(elmk_routing_heat_budget(ctx_, sums)); }
  void routing_heat_clear() { ok(elmk_routing_heat_clear(ctx_)); }
  /* Floodplain infiltration (elmk.h "floodplain infiltration"): the floodplain's water infiltrates the soil columns of its cell, and the
   * routing takes it out of WF.  floodplain_infiltration_enable() after soil_hydrology_enable, water_balance_enable,
   * routing_kinematic_enable and routing_inundation_enable, over an output grid with every column in at most one cell; soil_hydrology,
   * water_balance, routing and run() then take their forms with the term.  floodplain_infiltration_read() copies one of the column rows
   * ELMK_FPI_* ([ncols]), routing_read() takes ELMK_ROUTE_QLAND as well, floodplain_infiltration_budget() fills sums[1];
   * floodplain_infiltration_clear() returns to the stages without the term and keeps WF. */
  void floodplain_infiltration_enable() { ok(elmk_floodplain_infiltration_enable(ctx_)); }
  void floodplain_infiltration_read(int which, double* host) { ok(elmk_floodplain_infiltration_read(ctx_, which, host, 0, host ? ncols_ : 0)); }
  void floodplain_infiltration_budget(double* sums) { ok(elmk_floodplain_infiltration_budget(ctx_, sums)); }
  void floodplain_infiltration_clear() { ok(elmk_floodplain_infiltration_clear(ctx_)); }
  /* History entries over one fp64 row of a feature (elmk.h "feature rows on history tapes"): family ELMK_ROWS_*, which the family's
   * row number; as history_add / gridded_history_add otherwise, one level.  While such an entry exists the family's clear is refused. */
  int history_add_row(int tape, int family, int which, int op)
  {
    const int e = elmk_column_history_add_row(ctx_, tape, family, which, op);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  int gridded_history_add_row(int tape, int family, int which, int op)
  {
    const int e = elmk_gridded_history_add_row(ctx_, tape, family, which, op);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  /* A history entry over one fp64 CELL row of the river stages (elmk.h "cell rows on history tapes"): family ELMK_CELL_ROWS_ROUTING
   * (which = ELMK_ROUTE_*) or ELMK_CELL_ROWS_SUPPLY (ELMK_IRRSUP_*); every cell is a sample, history_read of it is [ncells].
   * run(..., routing = true, history = true) samples it after the step's routing.  While it exists the clear of its rows' owner
   * and the output grid's calls are refused. */
  int cell_history_add_row(int tape, int family, int which, int op)
  {
    const int e = elmk_cell_history_add_row(ctx_, tape, family, which, op);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  /* Point series (elmk.h "point series"): per-step records of chosen columns and river cells - a tower's series, a gauge's
   * hydrograph - in a device-resident ring.  points_set names the columns (ELMK_POINTS_COLUMNS) or the cells (ELMK_POINTS_CELLS),
   * points_add_* one source each (what the history entry points of the same kind accept), points_reserve the ring; then either
   * points_record(stamp) after a step, one launch, or points_set_run(true) and every step of run() records with its decday.
   * points_read gives one entry's [nrec][npoints], points_stamps the records' stamps, both oldest first. */
  void points_set(int kind, const std::vector<int64_t>& idx) { ok(elmk_points_set(ctx_, kind, (int64_t)idx.size(), idx.data())); }
  int points_add_field(const char* field, int level) { return entry(elmk_points_add_field(ctx_, id(field), level)); }
  int points_add_row(int family, int which) { return entry(elmk_points_add_row(ctx_, family, which)); }
  int points_add_cell_row(int family, int which) { return entry(elmk_points_add_cell_row(ctx_, family, which)); }
  int points_add_gridded_field(const char* field, int level) { return entry(elmk_points_add_gridded_field(ctx_, id(field), level)); }
  int points_add_gridded_row(int family, int which) { return entry(elmk_points_add_gridded_row(ctx_, family, which)); }
  void points_reserve(int max_records) { ok(elmk_points_reserve(ctx_, max_records)); }
  void points_record(double stamp) { ok(elmk_points_record(ctx_, stamp)); }
  void points_set_run(bool on) { ok(elmk_points_set_run(ctx_, on ? 1 : 0)); }
  int64_t points_count(int64_t* held = nullptr)
  {
    int64_t total = 0;
    ok(elmk_points_count(ctx_, &total, held));
    return total;
  }
  void points_read(int entry, double* host, int64_t rec0, int64_t nrec) { ok(elmk_points_read(ctx_, entry, host, rec0, nrec)); }
  void points_stamps(double* host, int64_t rec0, int64_t nrec) { ok(elmk_points_stamps(ctx_, host, rec0, nrec)); }
  void points_reset() { ok(elmk_points_reset(ctx_)); }
  void points_clear() { ok(elmk_points_clear(ctx_)); }
  /* ELMK_OPT_RESTART_CELLS (elmk.h "restart", version 6): saveRestart() / loadRestart() carry the river stages' state - VOLR, QOUT_SUM
   * and the call count, WH, WT, WF, UNMET_SUM - so that a restart needs no routing_init / ..._init call. */
  void restart_cells(bool on = true) { ok(elmk_set_option(ctx_, ELMK_OPT_RESTART_CELLS, on ? 1 : 0)); }

  /* Restart images (elmk.h "restart"): saveRestart() returns the image of the columns, global columns [gcol0, gcol0 + ncols);
   * loadRestart() takes one after setup, geography, maps and the same history and accumulator entries, in place of initialize().
   * Both throw on a refusal; the state is then untouched. */
  std::vector<unsigned char> saveRestart(int64_t gcol0 = 0)
  {
    int64_t bytes = 0;
    ok(elmk_restart_size(ctx_, &bytes));
    std::vector<unsigned char> image((size_t)bytes);
    ok(elmk_restart_save(ctx_, gcol0, image.data(), bytes));
    return image;
  }
  void loadRestart(const std::vector<unsigned char>& image, int64_t gcol0 = 0)
  {
    ok(elmk_restart_load(ctx_, gcol0, image.data(), (int64_t)image.size()));
  }

  /* Multi-step runs (elmk_run): the driver's time loop on the device.  reserve_run() once; the forcing records (atm_* fields, slots
   * 0 .. forcing_slots-1) and the 12 months of mlai .. mhbot go up as series, host[nslots][ncols], record-major; run() then does
   * advance() (the overload with solar geometry) for every row of the schedule, with no host round trip between steps, and throws if
   * a step raised a fatal flag.  enqueue_run() + finish_run() split run() in two: a series_upload() of records the run does not read
   * overlaps the run in between.  conservation() is the last step's triples, run_conservation() all of them ([nsteps][8][3]). */
  void reserve_run(int forcing_slots, int max_steps)
  {
    ok(elmk_run_reserve(ctx_, forcing_slots, max_steps));
    max_steps_ = max_steps;
  }
  void series_upload(const char* field, int slot0, int nslots, const double* host)
  {
    ok(elmk_series_upload(ctx_, id(field), slot0, nslots, host, 0, ncols_));
  }
  void enqueue_run(double dt_seconds, const std::vector<elmk_run_step>& steps, bool accumulate_history = false, bool qbot_rh = false,
                   bool update_accum = false, bool update_aerosol = false, bool update_active_layer = false, bool soil_hydrology = false,
                   bool water_balance = false, bool irrigation = false, bool routing = false)
  {
    ok(elmk_run(ctx_, dt_seconds, steps.data(), (int)steps.size(),
                (accumulate_history ? ELMK_RUN_HISTORY : 0) | (qbot_rh ? ELMK_RUN_QBOT_IS_RH : 0) | (update_accum ? ELMK_RUN_ACCUM : 0) |
                    (update_aerosol ? ELMK_RUN_AEROSOL : 0) | (update_active_layer ? ELMK_RUN_ALT : 0) |
                    (soil_hydrology ? ELMK_RUN_HYDROLOGY : 0) | (water_balance ? ELMK_RUN_WATER_BALANCE : 0) |
                    (irrigation ? ELMK_RUN_IRRIGATION : 0) | (routing ? ELMK_RUN_ROUTING : 0)));
  }
  bool finish_run()
  {
    const size_t m = (size_t)std::max(max_steps_, 1);
    std::vector<double> cons(m * 24);
    std::vector<uint32_t> flags(m);
    std::vector<int64_t> first(m);
    const int n = elmk_run_diagnostics(ctx_, cons.data(), flags.data(), first.data());
    ok(n < 0 ? n : ELMK_OK);
    run_conservation_.assign(cons.begin(), cons.begin() + (size_t)n * 24);
    if (n > 0) {  // (kept even when a step failed, as the Python mirror keeps them)
      std::copy(run_conservation_.end() - 24, run_conservation_.end(), &conservation_[0][0]);
      last_flags_ = flags[(size_t)n - 1];
    }
    for (int s = 0; s < n; s++)
      if (flags[(size_t)s] & ELMK_ERR_FATAL_MASK)
        throw std::runtime_error("ELM physics error flags " + std::to_string(flags[(size_t)s]) + " in step " + std::to_string(s) +
                                 " of the run, first at column " + std::to_string(first[(size_t)s]));
    return false;
  }
  bool run(double dt_seconds, const std::vector<elmk_run_step>& steps, bool accumulate_history = false, bool qbot_rh = false,
           bool update_accum = false, bool update_aerosol = false, bool update_active_layer = false, bool soil_hydrology = false,
           bool water_balance = false, bool irrigation = false, bool routing = false)
  {
    enqueue_run(dt_seconds, steps, accumulate_history, qbot_rh, update_accum, update_aerosol, update_active_layer, soil_hydrology, water_balance,
                irrigation, routing);
    return finish_run();
  }
  const std::vector<double>& run_conservation() const { return run_conservation_; }

  /* Aerosol deposition (elmk.h "aerosol deposition"; ELM's aerdepini / aerinterp, the hook the reference leaves commented out at
   * init_timestep_kokkos.cc:48-49): aerosol_reserve() allocates the twelve months of the eleven streams aer_bcphi .. aer_dst4_2 on
   * the aerosol file's own grid of ncells cells, with the map idx[npts][ncols] / w[npts][ncols] from that grid to the columns (both
   * nullptr: per-column series, ncells = ncols); aerosol_upload() fills months [month0, month0 + nmonths) of one stream from
   * host[nmonths][ncells].  update_aerosol() before advance() writes the eleven fields from the month bracket that also feeds
   * advance()'s month weights; run(..., update_aerosol = true) does it in every step from the step's month1 / month2 / weights. */
  void aerosol_reserve(int64_t ncells, int npts, const int32_t* idx, const double* w) { ok(elmk_aerosol_reserve(ctx_, ncells, npts, idx, w)); }
  void aerosol_upload(const char* field, int month0, int nmonths, const double* host)
  {
    ok(elmk_aerosol_upload(ctx_, id(field), month0, nmonths, host));
  }
  void update_aerosol(int month1, int month2, double wt1, double wt2) { ok(elmk_aerosol_deposition(ctx_, month1, month2, wt1, wt2)); }
  void aerosol_clear() { ok(elmk_aerosol_clear(ctx_)); }

  /* Forcing on a coarser grid (elmk_set_forcing_grid): the per-column map idx[npts][ncols] / w[npts][ncols] over ncells source
   * cells.  upload_gridded() remaps one level of an fp64 field from cells[ncells] on the device (the stepwise driver's path);
   * after reserve_run() the forcing series hold cell records, filled by series_upload_cells(), host[nslots][ncells].  Setting or
   * clearing the map releases the run reservation: reserve_run() again. */
  void set_forcing_grid(int64_t ncells, int npts, const int32_t* idx, const double* w)
  {
    ok(elmk_set_forcing_grid(ctx_, ncells, npts, idx, w));
    grid_ncells_ = ncells;
  }
  void clear_forcing_grid()
  {
    ok(elmk_clear_forcing_grid(ctx_));
    grid_ncells_ = 0;
  }
  void upload_gridded(const char* field, int level, const double* cells) { ok(elmk_upload_gridded(ctx_, id(field), level, cells)); }
  void series_upload_cells(const char* field, int slot0, int nslots, const double* host)
  {
    ok(elmk_series_upload(ctx_, id(field), slot0, nslots, host, 0, grid_ncells_));
  }
  int64_t grid_ncells() const { return grid_ncells_; }

  /* Output on a grid (elmk_set_output_grid): the CSR map by output cell - cell i averages columns col[ptr[i] .. ptr[i+1]-1] with
   * weights w (ELM's c2g, elmkernels_amd/regrid.py owner_map) - and fill for a cell without columns.  download_gridded() gives one
   * level of a field on the cells, [ncells]; gridded_history_add() registers a field on a tape with its accumulators on the cells,
   * folded by accumulate_history() and by run(..., accumulate_history = true); gridded_history_read() fills [ncells][nlev]. */
  void set_output_grid(int64_t ncells, const int64_t* ptr, const int32_t* col, const double* w, double fill)
  {
    ok(elmk_set_output_grid(ctx_, ncells, ptr, col, w, fill));
    output_ncells_ = ncells;
  }
  void clear_output_grid()
  {
    ok(elmk_clear_output_grid(ctx_));
    output_ncells_ = 0;
  }
  void download_gridded(const char* field, int level, double* cells) { ok(elmk_download_gridded(ctx_, id(field), level, cells)); }
  int gridded_history_add(int tape, const char* field, int op)
  {
    const int e = elmk_gridded_history_add(ctx_, tape, id(field), op);
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  void gridded_history_read(int entry, double* host)
  {
    ok(elmk_history_read(ctx_, entry, host, 0, output_ncells_, ELMK_LAYOUT_COL_MAJOR));
  }
  int64_t output_ncells() const { return output_ncells_; }

  /* ELMInterface::copyPrimaryVars / getPrimaryVars (elm_kokkos_interface.cc:324-356) */
  void copyPrimaryVars(PrimaryVars& pv)
  {
    download("snl", pv.snl.data());
    download("snow_depth", pv.snow_depth.data());
    download("frac_sno", pv.frac_sno.data());
    download("int_snow", pv.int_snow.data());
    download("snw_rds", pv.snw_rds.data());
    download("h2osoi_liq", pv.h2osoi_liq.data());
    download("h2osoi_ice", pv.h2osoi_ice.data());
    download("h2osoi_vol", pv.h2osoi_vol.data());
    download("h2ocan", pv.h2ocan.data());
    download("h2osno", pv.h2osno.data());
    download("h2osfc", pv.h2osfc.data());
    download("t_soisno", pv.t_soisno.data());
    download("t_grnd", pv.t_grnd.data());
    download("t_h2osfc", pv.t_h2osfc.data());
    download("t_h2osfc_bef", pv.t_h2osfc_bef.data());
    download("nrad", pv.nrad.data());
    download("dz", pv.dz.data());
    download("zsoi", pv.zsoi.data());
    download("zisoi", pv.zisoi.data());
  }
  std::shared_ptr<PrimaryVars> getPrimaryVars()
  {
    auto pv = std::make_shared<PrimaryVars>(ncols_);
    copyPrimaryVars(*pv);
    return pv;
  }

  /* (min, max, sum) of the eight conservation diagnostics of the last advance() (the reference prints column 0's) */
  const double (&conservation() const)[8][3] { return conservation_; }
  uint32_t warning_flags() const { return last_flags_; }  // ELMK_WARN_* bits raised in the last step
  elmk_ctx* context() { return ctx_; }
  int64_t ncols() const { return ncols_; }

 private:
  void ok(int rc)
  {
    if (rc != ELMK_OK) throw std::runtime_error(elmk_last_error(ctx_));
  }
  int entry(int e)  // an entry id, or a negative code
  {
    ok(e < 0 ? e : ELMK_OK);
    return e;
  }
  int id(const char* field)
  {
    const int f = elmk_field_id(field);
    if (f < 0) throw std::runtime_error(std::string("unknown ELM state field ") + field);
    return f;
  }
  elmk_ctx* ctx_{nullptr};
  int64_t ncols_{0};
  double conservation_[8][3]{};
  uint32_t last_flags_{0};
  int max_steps_{0};
  bool irrigation_{false};  // irrigation_enable(): advance() takes the split form
  int tod_{0};              // seconds after midnight UTC at the start of the next advance()
  int64_t grid_ncells_{0};
  int64_t routing_ncells_{0};
  int64_t output_ncells_{0};
  std::vector<double> run_conservation_;
};

}  // namespace elmk
