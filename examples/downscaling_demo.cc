// downscaling_demo.cc - forcing adjusted to column elevation (include/elmk.h "downscaling"), through include/elmk_interface.hpp:
// valley columns at the forcing cell's surface height beside mountain columns 1 500 m above it, all in one forcing cell and driven by
// the same near-freezing records, for one day of 48 half-hour steps as two runs of 24, once with downscaling OFF and once in TOPO mode
// (longwave renormalised over the cell: one group of every column, equal weights).  History tape 0 averages forc_tbot over the day;
// the demo prints the day's mean air temperature and the snow (h2osno) at the end of the day, valley beside mountain.  OFF gives every
// column the cell's air, so valley and mountain end alike; TOPO cools the mountain by the lapse rate, its precipitation falls as snow
// and the snowpack builds there.
// The input is the flat binary file of examples/run_demo.cc with 25 hourly records in the atm_* series (identical for every column),
// "topo" (each column's elevation, m), "hf" (the cell's surface height, m) and "steps" (48 elmk_run_step rows), written by
// tests/test_gpu_downscaling.py::test_downscaling_demo; examples/demo_io.h reads it.
//
//   g++ -std=c++17 -Iinclude examples/downscaling_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o downscaling_demo
//   ./downscaling_demo state.bin
#include <cstdio>
#include <vector>

#include "demo_io.h"

using namespace demo;
constexpr int NREC = 25, NSTEPS = 48, WINDOW = 24;

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
    const double* topo = in.D("topo");
    const double hf_cell = in.D("hf")[0];
    // every column sees the one cell's surface height; one longwave group over the cell
    const std::vector<double> hf((size_t)ncols, hf_cell), gw((size_t)ncols, 1.0 / (double)ncols);
    const std::vector<int64_t> gptr = {0, ncols};
    std::vector<int32_t> gcol((size_t)ncols);
    for (int64_t c = 0; c < ncols; c++) gcol[(size_t)c] = (int32_t)c;

    for (const int mode : {ELMK_DS_OFF, ELMK_DS_TOPO}) {
      elmk::ELMInterface elm(ncols, 0);
      setup(elm, in);
      upload_fields(elm, in);
      elm.set_column_geography(in.D("lat"), in.D("lon"));
      elm.set_column_elevation(topo, hf.data());
      elm.set_downscaling_groups(1, gptr.data(), gcol.data(), gw.data());
      elm.set_downscaling(mode);
      const int tbot = elm.history_add(0, "forc_tbot", ELMK_HIST_AVG);
      elm.reserve_run(NREC, WINDOW);
      upload_series(elm, in, NREC);
      elm.run(dt, first, true);
      elm.run(dt, second, true);
      std::vector<double> ta((size_t)ncols), sno((size_t)ncols);
      elm.history_read(tbot, ta.data());
      elm.download("h2osno", sno.data());
      double t_lo = 0.0, t_hi = 0.0, s_lo = 0.0, s_hi = 0.0;
      int64_t n_lo = 0, n_hi = 0;
      for (int64_t c = 0; c < ncols; c++) {
        if (topo[c] == hf_cell) {
          t_lo += ta[(size_t)c];
          s_lo += sno[(size_t)c];
          n_lo++;
        } else {
          t_hi += ta[(size_t)c];
          s_hi += sno[(size_t)c];
          n_hi++;
        }
      }
      if (!n_lo || !n_hi) throw std::runtime_error("need valley columns (topo == hf) and mountain columns");
      t_lo /= (double)n_lo, t_hi /= (double)n_hi, s_lo /= (double)n_lo, s_hi /= (double)n_hi;
      const char* verdict = mode == ELMK_DS_OFF ? (s_lo == s_hi && t_lo == t_hi ? "valley and mountain alike" : "NOT ALIKE")
                                                : (s_hi > s_lo && t_hi < t_lo ? "more snow on the mountain" : "NO MORE SNOW ON THE MOUNTAIN");
      std::printf("%s: %s: mean forc_tbot valley %.3f K, mountain %.3f K; h2osno valley %.3f, mountain %.3f kg/m2\n",
                  mode == ELMK_DS_OFF ? "off" : "topo", verdict, t_lo, t_hi, s_lo, s_hi);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "downscaling_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
