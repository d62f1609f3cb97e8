// accum_demo.cc - ELM's T10 kept on the device (elmk.h "accumulated fields") through include/elmk_interface.hpp: 48 half-hour steps
// as ONE run whose every step folds t_ref2m into a running mean over 8 steps and writes it to t10, the field photosynthesis reads
// for its acclimation terms.  The result is set against the loop this replaces - one run per step, and between two steps the host
// downloads t_ref2m, applies the update and uploads t10 - and against a run that leaves t10 at its start-up value.  The demo prints
// whether the first two are bit-identical (restart images, the accumulator and its step count) and how far t10 has moved.  Input:
// the state.bin of examples/run_demo.cc (written by tests/test_gpu_run.py::test_run_demo and tests/test_gpu_accum.py::test_accum_demo);
// examples/demo_io.h reads it and starts a context up.
//
//   g++ -std=c++17 -Iinclude examples/accum_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o accum_demo
//   ./accum_demo state.bin
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_io.h"

using namespace demo;
constexpr int NREC = 25, NSTEPS = 48;
constexpr int64_t PERIOD = 8;  // steps of the running mean (ELM: ten days)

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
    const double dt = in.dt();
    const size_t n = (size_t)ncols;

    // on the device: the value starts from the t10 that was uploaded, as a window that is already full
    elmk::ELMInterface device(ncols, 0);
    start(device, in, NREC, NSTEPS);
    const int entry = device.accum_add("t_ref2m", ELMK_ACCUM_RUNMEAN, PERIOD, "t10");
    device.accum_init(entry, nullptr, PERIOD);
    device.run(dt, steps, false, false, true);
    std::vector<double> val(n);
    const int64_t count = device.accum_read(entry, val.data());

    // the loop it replaces: a round trip through the host after every step
    elmk::ELMInterface host(ncols, 0);
    start(host, in, NREC, NSTEPS);
    std::vector<double> t10(n), tref(n);
    host.download("t10", t10.data());
    for (int s = 0; s < NSTEPS; s++) {
      host.run(dt, std::vector<elmk_run_step>(1, steps[(size_t)s]));
      host.download("t_ref2m", tref.data());
      const int64_t a = std::min<int64_t>(PERIOD + s + 1, PERIOD);
      for (size_t c = 0; c < n; c++) {
        const double prod = (double)(a - 1) * t10[c];
        const double sum = prod + tref[c];
        t10[c] = sum / (double)a;
      }
      host.upload("t10", t10.data());
    }

    // and t10 left alone
    elmk::ELMInterface frozen(ncols, 0);
    start(frozen, in, NREC, NSTEPS);
    frozen.run(dt, steps);
    std::vector<double> t10_frozen(n);
    frozen.download("t10", t10_frozen.data());

    device.accum_clear();  // (a context without entries saves the image the host loop's context saves)
    const bool same_state = device.saveRestart() == host.saveRestart();
    const bool same_val = std::memcmp(val.data(), t10.data(), n * sizeof(double)) == 0 && count == PERIOD + NSTEPS;
    double moved = 0.0;
    for (size_t c = 0; c < n; c++) moved = std::max(moved, std::fabs(val[c] - t10_frozen[c]));
    std::printf("t10 as a running mean over %lld steps, %d steps on %lld columns: device vs host round trips %s; t10 moved by up to %.3f K\n",
                (long long)PERIOD, NSTEPS, (long long)ncols, same_state && same_val ? "bit-identical" : "DIFFERENT", moved);
    return same_state && same_val && moved > 0.0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "accum_demo: %s\n", e.what());
    return 1;
  }
}
