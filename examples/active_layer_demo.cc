// active_layer_demo.cc - ELM's active layer thickness kept on the device (elmk.h "active layer thickness") through
// include/elmk_interface.hpp: a short run of half-hour steps across 00:00 of 1 January as ONE run whose every step computes the depth
// of the thaw front from t_soisno, keeps the annual maximum and, on the step that starts the new year, rolls the maximum of the
// northern columns over into last year's.  The result is set against the loop this replaces - one run per step and a stepwise
// update_active_layer() with the rollover bits the driver derives from the date - and the three rows ALT, ALTMAX and ALTMAX_LASTYEAR
// of a few columns are printed with the two layer indices.  Input: the state.bin of examples/run_demo.cc with a schedule that crosses
// the new year (written by tests/test_gpu_active_layer.py::test_active_layer_demo); examples/demo_io.h reads it.
//
//   g++ -std=c++17 -Iinclude examples/active_layer_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o active_layer_demo
//   ./active_layer_demo state.bin
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_io.h"

constexpr int NREC = 25;

// start-up as every run demo's, then a cold start of the feature
static void start(elmk::ELMInterface& elm, const demo::Inputs& in, int nsteps)
{
  demo::start(elm, in, NREC, nsteps);
  elm.active_layer_enable();
  const std::vector<int32_t> none((size_t)in.ncols, -1);  // no thawed layer seen yet
  elm.upload("altmax_indx", none.data());
  elm.upload("altmax_lastyear_indx", none.data());
}

struct Rows {
  std::vector<double> row[3];
  std::vector<int32_t> indx, indx_lastyear;
  void read(elmk::ELMInterface& elm, size_t n)
  {
    for (int w = 0; w < 3; w++) {
      row[w].resize(n);
      elm.active_layer_read(w, row[w].data());
    }
    indx.resize(n);
    indx_lastyear.resize(n);
    elm.download("altmax_indx", indx.data());
    elm.download("altmax_lastyear_indx", indx_lastyear.data());
  }
  bool operator==(const Rows& o) const
  {
    for (int w = 0; w < 3; w++)
      if (std::memcmp(row[w].data(), o.row[w].data(), row[w].size() * sizeof(double)) != 0) return false;
    return indx == o.indx && indx_lastyear == o.indx_lastyear;
  }
};

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin\n", argv[0]);
    return 2;
  }
  try {
    const demo::Inputs in(argv[1]);
    const int64_t ncols = in.ncols;
    const std::vector<elmk_run_step> steps = demo::run_steps(in);  // as many as the file holds
    const int nsteps = (int)steps.size();
    const double dt = in.dt();
    const double* lat = in.D("lat");
    const size_t n = (size_t)ncols;

    // on the device: every step of one run
    elmk::ELMInterface device(ncols, 0);
    start(device, in, nsteps);
    device.run(dt, steps, false, false, false, false, true);
    Rows got;
    got.read(device, n);

    // the loop it replaces: one run per step, then the update with the rollover bits of the step's start date
    elmk::ELMInterface host(ncols, 0);
    start(host, in, nsteps);
    int rolled = 0;
    for (int s = 0; s < nsteps; s++) {
      const elmk_run_step& q = steps[(size_t)s];
      host.run(dt, std::vector<elmk_run_step>(1, q));
      const int roll = (q.doy == 0 && q.decday == 1.0 ? ELMK_ALT_ROLL_NORTH : 0) | (q.doy == 181 && q.decday == 182.0 ? ELMK_ALT_ROLL_SOUTH : 0);
      rolled += roll != 0;
      host.update_active_layer(roll);
    }
    Rows want;
    want.read(host, n);

    const bool same = got == want;
    std::printf("active layer thickness, %d steps on %lld columns, %d rollover step(s): one run vs stepwise updates %s\n", nsteps,
                (long long)ncols, rolled, same ? "bit-identical" : "DIFFERENT");
    std::printf("%8s %8s %10s %10s %16s %6s %6s\n", "column", "lat", "ALT", "ALTMAX", "ALTMAX_LASTYEAR", "indx", "lastyr");
    for (size_t c = 0; c < n; c += std::max<size_t>(1, n / 6))
      std::printf("%8zu %8.3f %10.4f %10.4f %16.4f %6d %6d\n", c, lat[c], got.row[ELMK_ALT_ALT][c], got.row[ELMK_ALT_ALTMAX][c],
                  got.row[ELMK_ALT_ALTMAX_LASTYEAR][c], (int)got.indx[c], (int)got.indx_lastyear[c]);
    return same && rolled == 1 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "active_layer_demo: %s\n", e.what());
    return 1;
  }
}
