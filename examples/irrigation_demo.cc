// irrigation_demo.cc - the irrigation stage of elmk.h ("irrigation") through the C ABI: a dry crop column through two days of half-hour
// steps.  Only the stage and the soil hydrology run on the device; what the rest of the physics would supply is done on the host in
// the plainest way: btran from the soil water by calc_root_moist_stress's formula, and the water on the ground (qflx_rain_grnd) handed
// to the soil as qflx_top_soil, which is what snow_hydrology does on a snow-free column.  In a model run elmk_run with
// ELMK_RUN_IRRIGATION | ELMK_RUN_HYDROLOGY does all of it in every step.  Prints btran, RATE, NLEFT and QFLX_IRRIG of column 0 around
// 06:00 local time of both days: on the first morning the check finds the root zone dry, sets the rate and the eight steps of the
// four-hour window count down; by the second morning the column is no longer stressed and nothing is applied.
//
//   g++ -std=c++17 -Iinclude examples/irrigation_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o irrigation_demo
//   ./irrigation_demo
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "elmk.h"

static elmk_ctx* ctx;
static void chk(int rc, const char* what)
{
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + elmk_last_error(ctx));
}
static int fid(const char* name)
{
  const int f = elmk_field_id(name);
  if (f < 0) throw std::runtime_error(std::string("no field ") + name);
  return f;
}
// one value per level for every column, [column][level]
static void put(const char* name, int64_t n, const std::vector<double>& levels)
{
  std::vector<double> a((size_t)n * levels.size());
  for (int64_t c = 0; c < n; c++)
    for (size_t l = 0; l < levels.size(); l++) a[(size_t)c * levels.size() + l] = levels[l];
  chk(elmk_upload(ctx, fid(name), a.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), name);
}
static void put_int(const char* name, int64_t n, int32_t v)
{
  std::vector<int32_t> a((size_t)n, v);
  chk(elmk_upload(ctx, fid(name), a.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), name);
}

int main()
{
  try {
    const int64_t n = 3;
    const double dt = 1800.0, watsat = 0.45, sucsat = 200.0, bsw = 5.0, smpso = -66000.0, smpsc = -255000.0;
    const int nsteps = 96, vtype = 17;
    const double londeg[n] = {0.0, 90.0, -120.0};
    chk(elmk_create(n, 0, &ctx), "elmk_create");
    chk(elmk_set_land(ctx, 2 /* crop */, 1, vtype, 0, 0), "elmk_set_land");
    // of the PFT tables the stage reads smpso only
    std::vector<double> psn((size_t)ELMK_MXPFT * ELMK_PSN_NPARAM, 0.0), alb((size_t)ELMK_MXPFT * ELMK_ALB_NPARAM, 0.0), z0mr(ELMK_MXPFT, 0.0),
        displar(ELMK_MXPFT, 0.0);
    for (int p = 0; p < ELMK_MXPFT; p++) {
      psn[(size_t)p * ELMK_PSN_NPARAM + 24] = smpso;
      psn[(size_t)p * ELMK_PSN_NPARAM + 25] = smpsc;
    }
    chk(elmk_set_pft(ctx, psn.data(), alb.data(), z0mr.data(), displar.data()), "elmk_set_pft");
    // ELM's soil grid: 5 snow levels (unused here), 15 ground layers
    std::vector<double> zi(21, 0.0), dz(20, 0.0), z(20, 0.0);
    for (int j = 0; j < 15; j++) z[5 + j] = 0.025 * (std::exp(0.5 * (j + 0.5)) - 1.0);
    for (int j = 0; j < 15; j++) zi[6 + j] = j < 14 ? 0.5 * (z[5 + j] + z[6 + j]) : z[19] + 0.5 * (z[19] - z[18]);
    for (int j = 0; j < 15; j++) dz[5 + j] = zi[6 + j] - zi[5 + j];
    std::vector<double> liq(20, 0.0), rootfr(15, 0.0);
    for (int j = 0; j < 15; j++) liq[5 + j] = 0.25 * watsat * dz[5 + j] * 1000.0;  // a quarter saturated
    const double roots[6] = {0.3, 0.25, 0.2, 0.12, 0.08, 0.05};
    for (int j = 0; j < 6; j++) rootfr[j] = roots[j];
    put("zisoi", n, zi);
    put("dz", n, dz);
    put("zsoi", n, z);
    put("h2osoi_liq", n, liq);
    put("h2osoi_ice", n, std::vector<double>(20, 0.0));
    put("t_soisno", n, std::vector<double>(20, 290.0));
    put("watsat", n, std::vector<double>(15, watsat));
    put("eff_porosity", n, std::vector<double>(15, watsat));  // no ice
    put("sucsat", n, std::vector<double>(15, sucsat));
    put("bsw", n, std::vector<double>(15, bsw));
    put("rootfr", n, rootfr);
    put("elai", n, {2.0});
    put_int("frac_veg_nosno", n, 1);
    put_int("vtype", n, vtype);

    chk(elmk_soil_hydrology_enable(ctx), "elmk_soil_hydrology_enable");
    std::vector<double> hksat((size_t)ELMK_HYD_NLAYER * n, 5.0e-2), wtfact(n, 0.0), thresh(n, 5.0), k_wet(n, 0.035), rsub(n, 0.0);
    chk(elmk_soil_hydrology_set_params(ctx, hksat.data(), wtfact.data(), thresh.data(), k_wet.data(), rsub.data()), "set_params");
    std::vector<double> zwt0(n, 6.0), wa0(n, 4000.0);
    chk(elmk_soil_hydrology_init(ctx, zwt0.data(), wa0.data()), "elmk_soil_hydrology_init");

    // the schedule: ELM's round(londeg / degpsec), degpsec = 15 / 3600, reduced to 0 .. 86399
    std::vector<int32_t> sched(n);
    for (int64_t c = 0; c < n; c++) sched[c] = (int32_t)(((std::llround(londeg[c] / (15.0 / 3600.0)) % 86400) + 86400) % 86400);
    chk(elmk_irrigation_enable(ctx, sched.data()), "elmk_irrigation_enable");

    std::vector<double> l((size_t)n * 20), btran(n), rate(n), nleft(n), qirr(n), ground(n), zero(n, 0.0);
    double applied = 0.0;
    std::printf("irrigation, %d steps of %.0f s, column 0 at longitude %.0f\n", nsteps, dt, londeg[0]);
    std::printf("%4s %6s %9s %12s %6s %12s\n", "step", "local", "btran", "RATE mm/s", "NLEFT", "QIRRIG mm/s");
    for (int s = 0; s < nsteps; s++) {
      const int tod = (int)((long long)s * (long long)dt % 86400);
      // what the physics would leave: btran of the current soil water, and a fresh qflx_rain_grnd (no rain)
      chk(elmk_download(ctx, fid("h2osoi_liq"), l.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
      for (int64_t c = 0; c < n; c++) {
        double b = 0.0;
        for (int j = 0; j < 15; j++) {
          const double sn = std::fmax(std::fmin(l[(size_t)c * 20 + 5 + j] / (dz[5 + j] * 1000.0), watsat) / watsat, 0.01);
          const double smp = std::fmax(smpsc, -sucsat * std::pow(sn, -bsw));
          b += rootfr[j] * std::fmin((smp - smpsc) / (smpso - smpsc), 1.0);
        }
        btran[c] = b;
      }
      chk(elmk_upload(ctx, fid("btran"), btran.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "btran");
      chk(elmk_upload(ctx, fid("qflx_rain_grnd"), zero.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "qflx_rain_grnd");
      chk(elmk_irrigation(ctx, dt, tod), "elmk_irrigation");
      chk(elmk_download(ctx, fid("qflx_rain_grnd"), ground.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
      chk(elmk_upload(ctx, fid("qflx_top_soil"), ground.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "qflx_top_soil");
      chk(elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      chk(elmk_irrigation_read(ctx, ELMK_IRR_RATE, rate.data(), 0, n), "read");
      chk(elmk_irrigation_read(ctx, ELMK_IRR_NLEFT, nleft.data(), 0, n), "read");
      chk(elmk_irrigation_read(ctx, ELMK_IRR_QFLX_IRRIG, qirr.data(), 0, n), "read");
      applied += qirr[0] * dt;
      const int local = (tod + sched[0]) % 86400;
      if (local >= 5 * 3600 && local <= 10 * 3600 + 1800)
        std::printf("%4d %3d:%02d %9.6f %12.5e %6.0f %12.5e\n", s, local / 3600, local % 3600 / 60, btran[0], rate[0], nleft[0], qirr[0]);
    }
    std::printf("applied to column 0: %.3f mm\n", applied);
    chk(elmk_destroy(ctx), "elmk_destroy");
    return applied > 0.0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "irrigation_demo: %s\n", e.what());
    return 1;
  }
}
