// shortwave_demo.cc - incident shortwave from interval-mean forcing records (include/elmk.h "shortwave"), through
// include/elmk_interface.hpp: one day of 48 half-hour steps over 3-hourly FSDS records, as two runs of 24, once in each shortwave
// mode.  History tape 0 averages forc_solad and forc_solai over the day; the demo prints the domain's mean incident shortwave
// beside the records' mean.  In REFERENCE mode (the reference's ProcessFSDS) a column receives the record times the step's mean
// cos(zenith), which falls short of the records; in COSZEN mode ELM's factor spreads each record over the steps of its interval and
// the day receives what the records hold (up to the steps where cos(zenith) is at most 0.001 or the factor is capped at 10).
// The input is the flat binary file of examples/run_demo.cc with 9 three-hourly records in the atm_* series, "recs" (the record
// starts, decimal_doy + 1.0) and "steps" (48 elmk_run_step rows), written by tests/test_gpu_shortwave.py::test_shortwave_demo_runs;
// examples/demo_io.h reads it.
//
//   g++ -std=c++17 -Iinclude examples/shortwave_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o shortwave_demo
//   ./shortwave_demo state.bin
#include <cmath>
#include <cstdio>
#include <vector>

#include "demo_io.h"

using namespace demo;
constexpr int NREC = 9, NSTEPS = 48, WINDOW = 24;
constexpr double FORC_DT = 3 * 3600.0;

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin\n", argv[0]);
    return 2;
  }
  try {
    const Inputs in(argv[1]);
    const int64_t ncols = in.ncols;
    const std::vector<elmk_run_step> steps = run_steps(in, NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = in.dt();
    // the records' mean over the day: records 0 .. 7 (record 8 only brackets the last step)
    const double* fsds = in.D("series/atm_fsds");
    double rec_mean = 0.0;
    for (int r = 0; r < NREC - 1; r++)
      for (int64_t c = 0; c < ncols; c++) rec_mean += fsds[(size_t)r * ncols + c];
    rec_mean /= (double)(NREC - 1) * (double)ncols;

    for (const int mode : {ELMK_SW_REFERENCE, ELMK_SW_COSZEN}) {
      elmk::ELMInterface elm(ncols, 0);
      setup(elm, in);
      upload_fields(elm, in);
      elm.set_column_geography(in.D("lat"), in.D("lon"));
      elm.set_shortwave_mode(mode, FORC_DT);
      const int solad = elm.history_add(0, "forc_solad", ELMK_HIST_AVG), solai = elm.history_add(0, "forc_solai", ELMK_HIST_AVG);
      elm.reserve_run(NREC, WINDOW);
      upload_series(elm, in, NREC);
      if (mode == ELMK_SW_COSZEN) elm.series_record_times(0, NREC, in.D("recs"));
      elm.run(dt, first, true);
      elm.run(dt, second, true);
      std::vector<double> a((size_t)ncols * 2), b((size_t)ncols * 2);
      elm.history_read(solad, a.data());
      elm.history_read(solai, b.data());
      double day_mean = 0.0;
      for (size_t i = 0; i < a.size(); i++) day_mean += a[i] + b[i];
      day_mean /= (double)ncols;
      const double rel = day_mean / rec_mean - 1.0;
      if (mode == ELMK_SW_COSZEN)
        std::printf("coszen: %s: day's mean incident shortwave %.4f W/m2, records' mean %.4f W/m2 (%+.2e)\n",
                    std::fabs(rel) < 1e-2 ? "kept" : "NOT KEPT", day_mean, rec_mean, rel);
      else
        std::printf("reference: %s: day's mean incident shortwave %.4f W/m2, records' mean %.4f W/m2 (%+.2e)\n",
                    rel < -0.1 ? "short" : "not short", day_mean, rec_mean, rel);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shortwave_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
