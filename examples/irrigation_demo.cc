// irrigation_demo.cc - the irrigation stage of elmk.h ("irrigation") through the C ABI: a dry crop column through two days of half-hour
// steps.  Only the stage and the soil hydrology run on the device; what the rest of the physics would supply is done on the host in
// the plainest way: btran from the soil water by calc_root_moist_stress's formula, and the water on the ground (qflx_rain_grnd) handed
// to the soil as qflx_top_soil, which is what snow_hydrology does on a snow-free column.  In a model run elmk_run with
// ELMK_RUN_IRRIGATION | ELMK_RUN_HYDROLOGY does all of it in every step.  Prints btran, RATE, NLEFT and QFLX_IRRIG of column 0 around
// 06:00 local time of both days: on the first morning the check finds the root zone dry, sets the rate and the eight steps of the
// four-hour window count down; by the second morning the column is no longer stressed and nothing is applied.  The loam columns come
// from examples/demo_site.h.
//
//   g++ -std=c++17 -Iinclude examples/irrigation_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o irrigation_demo
//   ./irrigation_demo
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_site.h"

using namespace demo;

static void put_int(elmk_ctx* ctx, const char* name, int64_t n, int32_t v)
{
  std::vector<int32_t> a((size_t)n, v);
  chk(ctx, elmk_upload(ctx, fid(name), a.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), name);
}

int main()
{
  try {
    const int64_t n = 3;
    const double dt = 1800.0, smpso = -66000.0, smpsc = -255000.0;
    const int nsteps = 96, vtype = 17;
    const double londeg[n] = {0.0, 90.0, -120.0};
    elmk_ctx* ctx = nullptr;
    chk(ctx, elmk_create(n, 0, &ctx), "elmk_create");
    chk(ctx, elmk_set_land(ctx, 2 /* crop */, 1, vtype, 0, 0), "elmk_set_land");
    // of the PFT tables the stage reads smpso only
    std::vector<double> psn((size_t)ELMK_MXPFT * ELMK_PSN_NPARAM, 0.0), alb((size_t)ELMK_MXPFT * ELMK_ALB_NPARAM, 0.0), z0mr(ELMK_MXPFT, 0.0),
        displar(ELMK_MXPFT, 0.0);
    for (int p = 0; p < ELMK_MXPFT; p++) {
      psn[(size_t)p * ELMK_PSN_NPARAM + 24] = smpso;
      psn[(size_t)p * ELMK_PSN_NPARAM + 25] = smpsc;
    }
    chk(ctx, elmk_set_pft(ctx, psn.data(), alb.data(), z0mr.data(), displar.data()), "elmk_set_pft");
    loam_columns(ctx, n, 0.25);  // a quarter saturated
    std::vector<double> zi, dz, z, rootfr(15, 0.0);
    soil_grid(zi, dz, z);  // (dz: for btran below)
    const double roots[6] = {0.3, 0.25, 0.2, 0.12, 0.08, 0.05};
    for (int j = 0; j < 6; j++) rootfr[j] = roots[j];
    put(ctx, "t_soisno", n, std::vector<double>(20, 290.0));
    put(ctx, "eff_porosity", n, std::vector<double>(15, WATSAT));  // no ice
    put(ctx, "rootfr", n, rootfr);
    put(ctx, "elai", n, {2.0});
    put_int(ctx, "frac_veg_nosno", n, 1);
    put_int(ctx, "vtype", n, vtype);

    hydrology_on(ctx, n, 5.0e-2, /*wtfact=*/0.0, 0.035, /*rsub=*/0.0);
    hydrology_start(ctx, n, 6.0);

    // the schedule: ELM's round(londeg / degpsec), degpsec = 15 / 3600, reduced to 0 .. 86399
    std::vector<int32_t> sched(n);
    for (int64_t c = 0; c < n; c++) sched[c] = (int32_t)(((std::llround(londeg[c] / (15.0 / 3600.0)) % 86400) + 86400) % 86400);
    chk(ctx, elmk_irrigation_enable(ctx, sched.data()), "elmk_irrigation_enable");

    std::vector<double> l((size_t)n * 20), btran(n), rate(n), nleft(n), qirr(n), ground(n), zero(n, 0.0);
    double applied = 0.0;
    std::printf("irrigation, %d steps of %.0f s, column 0 at longitude %.0f\n", nsteps, dt, londeg[0]);
    std::printf("%4s %6s %9s %12s %6s %12s\n", "step", "local", "btran", "RATE mm/s", "NLEFT", "QIRRIG mm/s");
    for (int s = 0; s < nsteps; s++) {
      const int tod = (int)((long long)s * (long long)dt % 86400);
      // what the physics would leave: btran of the current soil water, and a fresh qflx_rain_grnd (no rain)
      chk(ctx, elmk_download(ctx, fid("h2osoi_liq"), l.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
      for (int64_t c = 0; c < n; c++) {
        double b = 0.0;
        for (int j = 0; j < 15; j++) {
          const double sn = std::fmax(std::fmin(l[(size_t)c * 20 + 5 + j] / (dz[5 + j] * 1000.0), WATSAT) / WATSAT, 0.01);
          const double smp = std::fmax(smpsc, -SUCSAT * std::pow(sn, -BSW));
          b += rootfr[j] * std::fmin((smp - smpsc) / (smpso - smpsc), 1.0);
        }
        btran[c] = b;
      }
      chk(ctx, elmk_upload(ctx, fid("btran"), btran.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "btran");
      chk(ctx, elmk_upload(ctx, fid("qflx_rain_grnd"), zero.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "qflx_rain_grnd");
      chk(ctx, elmk_irrigation(ctx, dt, tod), "elmk_irrigation");
      chk(ctx, elmk_download(ctx, fid("qflx_rain_grnd"), ground.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "download");
      chk(ctx, elmk_upload(ctx, fid("qflx_top_soil"), ground.data(), 0, n, ELMK_LAYOUT_COL_MAJOR), "qflx_top_soil");
      chk(ctx, elmk_soil_hydrology(ctx, dt), "elmk_soil_hydrology");
      chk(ctx, elmk_irrigation_read(ctx, ELMK_IRR_RATE, rate.data(), 0, n), "read");
      chk(ctx, elmk_irrigation_read(ctx, ELMK_IRR_NLEFT, nleft.data(), 0, n), "read");
      chk(ctx, elmk_irrigation_read(ctx, ELMK_IRR_QFLX_IRRIG, qirr.data(), 0, n), "read");
      applied += qirr[0] * dt;
      const int local = (tod + sched[0]) % 86400;
      if (local >= 5 * 3600 && local <= 10 * 3600 + 1800)
        std::printf("%4d %3d:%02d %9.6f %12.5e %6.0f %12.5e\n", s, local / 3600, local % 3600 / 60, btran[0], rate[0], nleft[0], qirr[0]);
    }
    std::printf("applied to column 0: %.3f mm\n", applied);
    chk(ctx, elmk_destroy(ctx), "elmk_destroy");
    return applied > 0.0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "irrigation_demo: %s\n", e.what());
    return 1;
  }
}
