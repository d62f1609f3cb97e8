// forcing_grid_demo.cc - the driver's time loop on the device with forcing on the data set's own grid: a day of half-hour steps over
// columns spread across the globe, driven by hourly records on a 64 x 32 cell grid that the device remaps to every column
// (include/elmk.h "forcing grid").  The host sends 2048 values per record and stream instead of one per column.  48 steps run as two
// runs of 24; the cell records of the second window go up while the first run executes.
// Input: the flat binary file of examples/run_demo.cc, with the forcing as cell records ("cells/<field>": [records][ncells], 25 hourly
// records for atm_*) and the remap map ("map/idx" int32 and "map/w" double, [npts][ncols], built by elmkernels_amd/regrid.py's
// bilinear_map), written by tests/test_gpu_forcing_grid.py::test_forcing_grid_demo; examples/demo_io.h reads it.
//
//   g++ -std=c++17 -Iinclude examples/forcing_grid_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o forcing_grid_demo
//   ./forcing_grid_demo state.bin [out.bin]
//
// out.bin: as run_demo's - the PrimaryVars members in ELMInterface order, then the 48 conservation rows [48][8][3] doubles.
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

    // the map: npts rows of ncols terms; ncells from the size of a cell record
    const int npts = (int)(in.sizes.at("map/idx") / (int64_t)(sizeof(int32_t) * ncols));
    if (in.sizes.at("map/w") != (int64_t)(sizeof(double)) * npts * ncols) throw std::runtime_error("map/w: expected [npts][ncols]");
    const int64_t ncells = in.sizes.at("cells/atm_tbot") / (int64_t)(sizeof(double) * NREC);
    elm.set_forcing_grid(ncells, npts, in.I("map/idx"), in.D("map/w"));

    const std::vector<elmk_run_step> steps = run_steps(in, NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = in.dt();

    // 25 cell records per forcing stream and the 12 months (per column) on the device; the first window's records (slots 0 .. 12)
    // before the first run.  The reservation comes after set_forcing_grid: it sizes the forcing series by cells.
    elm.reserve_run(NREC, WINDOW);
    const int split = first.back().forc_slot + 2;  // records the first run reads: 0 .. split - 1
    for (const char* f : FORCING) elm.series_upload_cells(f, 0, split, in.D(std::string("cells/") + f));
    for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, in.D(std::string("series/") + f));
    elm.enqueue_run(dt, first);
    // the second window goes up while the first run executes (it reads none of these records, so nothing waits)
    for (const char* f : FORCING) elm.series_upload_cells(f, split, NREC - split, in.D(std::string("cells/") + f) + (size_t)split * ncells);
    elm.finish_run();
    std::vector<double> cons = elm.run_conservation();
    elm.run(dt, second);
    cons.insert(cons.end(), elm.run_conservation().begin(), elm.run_conservation().end());

    const auto pv = elm.getPrimaryVars();
    std::printf("%d steps on %lld columns from %lld forcing cells (%d terms per column) in two runs: water balance error of the last "
                "step %.3e .. %.3e kg/m2\n", NSTEPS, (long long)ncols, (long long)ncells, npts, elm.conservation()[1][0],
                elm.conservation()[1][1]);
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
    std::fprintf(stderr, "forcing_grid_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
