// history_demo.cc - time-averaged output without a download per step, through include/elmk_interface.hpp: register a history tape
// of fluxes (average) and one of ground temperature extremes once, step a simulated day of half-hour steps (advance(), then
// accumulate_history(): one kernel launch per step, nothing crosses the host link), read every entry once at the end.
// The state and parameter arrays come from the flat binary file of examples/elm_interface_demo.cc (written by
// tests/test_gpu_history.py::test_history_demo_runs); examples/demo_io.h reads it and makes the setup() call.
//
//   g++ -std=c++17 -Iinclude examples/history_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o history_demo
//   ./history_demo state.bin [nsteps = 48] [out.bin]
//
// out.bin: the entries in the order of AVG_FIELDS, then t_grnd max, t_grnd min, each [ncols] doubles; then int64 sample counts of
// tapes 0 and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "demo_io.h"

// single-level fluxes of the averaged tape
static const char* const AVG_FIELDS[] = {"eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "eflx_soil_grnd", "fsa", "eflx_lwrad_out"};
constexpr int NAVG = sizeof AVG_FIELDS / sizeof AVG_FIELDS[0];

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin [nsteps] [out.bin]\n", argv[0]);
    return 2;
  }
  try {
    const demo::Inputs in(argv[1]);
    const int nsteps = argc > 2 ? std::atoi(argv[2]) : 48;
    const int64_t ncols = in.ncols;

    elmk::ELMInterface elm(ncols, 0);
    demo::setup(elm, in);
    demo::upload_fields(elm, in);

    // tape 0: daily means of the fluxes; tape 1: daily extremes of the ground temperature
    std::vector<int> entries;
    for (const char* f : AVG_FIELDS) entries.push_back(elm.history_add(0, f, ELMK_HIST_AVG));
    entries.push_back(elm.history_add(1, "t_grnd", ELMK_HIST_MAX));
    entries.push_back(elm.history_add(1, "t_grnd", ELMK_HIST_MIN));

    elmk::StepWeights w;
    std::memcpy(w.forc_wt1, in.D("forc_wt1"), 64);
    std::memcpy(w.forc_wt2, in.D("forc_wt2"), 64);
    w.month_wt1 = in.D("month_wt")[0];
    w.month_wt2 = in.D("month_wt")[1];
    w.qbot_is_relative_humidity = 0;
    const double dt = in.dt();
    for (int s = 0; s < nsteps; s++) {
      if (elm.advance(dt, w)) return 1;
      elm.accumulate_history();
    }

    // end of the output interval: one read per entry, then the tapes start the next interval
    std::vector<std::vector<double>> out(entries.size(), std::vector<double>((size_t)ncols));
    for (size_t k = 0; k < entries.size(); k++) elm.history_read(entries[k], out[k].data());
    const int64_t count0 = elm.history_count(0), count1 = elm.history_count(1);
    elm.history_reset(0);
    elm.history_reset(1);
    double mean_sh = 0.0, tmax = -1e300, tmin = 1e300;
    for (int64_t c = 0; c < ncols; c++) {
      mean_sh += out[0][(size_t)c] / (double)ncols;
      tmax = std::max(tmax, out[NAVG][(size_t)c]);
      tmin = std::min(tmin, out[NAVG + 1][(size_t)c]);
    }
    std::printf("history over %lld steps on %lld columns: domain mean of the mean sensible heat flux %.3f W/m2, t_grnd %.2f .. %.2f K\n",
                (long long)count0, (long long)ncols, mean_sh, tmin, tmax);
    if (count0 != nsteps || count1 != nsteps) throw std::runtime_error("unexpected sample count");
    if (argc > 3) {
      FILE* o = std::fopen(argv[3], "wb");
      if (!o) throw std::runtime_error(std::string("cannot open ") + argv[3]);
      for (const auto& v : out) std::fwrite(v.data(), 8, v.size(), o);
      std::fwrite(&count0, 8, 1, o);
      std::fwrite(&count1, 8, 1, o);
      std::fclose(o);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "history_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
