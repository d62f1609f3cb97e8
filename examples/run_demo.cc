// run_demo.cc - the driver's time loop on the device, through include/elmk_interface.hpp: a day of half-hour steps over a grid that
// spans latitudes and longitudes, driven by hourly forcing records and monthly phenology that stay on the GPU.  48 steps run as two
// runs of 24; the records of the second window go up while the first run executes, and no step waits for the host.
// The state and parameter arrays come from the flat binary file of examples/history_demo.cc, plus the geography ("lat", "lon"), the
// series ("series/<field>": [records][ncols], 25 hourly records for atm_*, 12 months for mlai .. mhbot) and the schedule ("steps":
// 48 elmk_run_step rows), written by tests/test_gpu_run.py::test_run_demo: the demo has no calendar of its own, and examples/demo_io.h
// reads the file and sets the context up.
//
//   g++ -std=c++17 -Iinclude examples/run_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o run_demo
//   ./run_demo state.bin [out.bin]
//
// out.bin: the PrimaryVars members in ELMInterface order (snl, snow_depth, frac_sno, int_snow, snw_rds, h2osoi_liq, h2osoi_ice,
// h2osoi_vol, h2ocan, h2osno, h2osfc, t_soisno, t_grnd, t_h2osfc, t_h2osfc_bef, nrad, dz, zsoi, zisoi), then the 48 conservation
// rows [48][8][3] doubles.
#include <cstdio>
#include <string>
#include <vector>

#include "demo_io.h"

using namespace demo;
constexpr int NREC = 25, NSTEPS = 48, WINDOW = 24;

template <class T> static void put(FILE* o, const std::vector<T>& v) { std::fwrite(v.data(), sizeof(T), v.size(), o); }

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin [out.bin]\n", argv[0]);
    return 2;
  }
  try {
    const Inputs in(argv[1]);
    const int64_t ncols = in.ncols;
    elmk::ELMInterface elm(ncols, 0);
    setup(elm, in);
    upload_fields(elm, in);
    elm.set_column_geography(in.D("lat"), in.D("lon"));

    const std::vector<elmk_run_step> steps = run_steps(in, NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = in.dt();

    // all 25 forcing slots and the 12 months on the device; the first window's records (slots 0 .. 12) before the first run
    elm.reserve_run(NREC, WINDOW);
    const int split = first.back().forc_slot + 2;  // records the first run reads: 0 .. split - 1
    for (const char* f : FORCING) elm.series_upload(f, 0, split, in.D(std::string("series/") + f));
    for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, in.D(std::string("series/") + f));
    elm.enqueue_run(dt, first);
    // the second window goes up while the first run executes (it reads none of these records, so nothing waits)
    for (const char* f : FORCING) elm.series_upload(f, split, NREC - split, in.D(std::string("series/") + f) + (size_t)split * ncols);
    elm.finish_run();
    std::vector<double> cons = elm.run_conservation();
    elm.run(dt, second);
    cons.insert(cons.end(), elm.run_conservation().begin(), elm.run_conservation().end());

    const auto pv = elm.getPrimaryVars();
    std::printf("%d steps on %lld columns in two runs: water balance error of the last step %.3e .. %.3e kg/m2\n", NSTEPS,
                (long long)ncols, elm.conservation()[1][0], elm.conservation()[1][1]);
    if (argc > 2) {
      FILE* o = std::fopen(argv[2], "wb");
      if (!o) throw std::runtime_error(std::string("cannot open ") + argv[2]);
      put(o, pv->snl);
      put(o, pv->snow_depth);
      put(o, pv->frac_sno);
      put(o, pv->int_snow);
      put(o, pv->snw_rds);
      put(o, pv->h2osoi_liq);
      put(o, pv->h2osoi_ice);
      put(o, pv->h2osoi_vol);
      put(o, pv->h2ocan);
      put(o, pv->h2osno);
      put(o, pv->h2osfc);
      put(o, pv->t_soisno);
      put(o, pv->t_grnd);
      put(o, pv->t_h2osfc);
      put(o, pv->t_h2osfc_bef);
      put(o, pv->nrad);
      put(o, pv->dz);
      put(o, pv->zsoi);
      put(o, pv->zisoi);
      put(o, cons);
      std::fclose(o);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "run_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
