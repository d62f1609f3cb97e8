// restart_demo.cc - an exact restart (E3SM's ERS test) through include/elmk_interface.hpp: 24 half-hour steps, saveRestart() to a
// file, the context destroyed; a new context set up as at start-up, loadRestart() from the file, 24 more steps.  The result is set
// against one continuous run of 48 steps and the demo prints whether the two are bit-identical (their restart images and the last
// step's conservation diagnostics).  Input: the state.bin of examples/run_demo.cc (written by tests/test_gpu_run.py::test_run_demo,
// and by tests/test_gpu_restart.py::test_restart_demo); examples/demo_io.h reads it and starts a context up.
//
//   g++ -std=c++17 -Iinclude examples/restart_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o restart_demo
//   ./restart_demo state.bin restart.img
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_io.h"

using namespace demo;
constexpr int NREC = 25, NSTEPS = 48, WINDOW = 24;

int main(int argc, char** argv)
{
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s state.bin restart.img\n", argv[0]);
    return 2;
  }
  try {
    const Inputs in(argv[1]);
    const int64_t ncols = in.ncols;
    const std::vector<elmk_run_step> steps = run_steps(in, NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = in.dt();

    {  // the first half, saved to a file; the context ends with the scope
      elmk::ELMInterface elm(ncols, 0);
      start(elm, in, NREC, NSTEPS);
      elm.run(dt, first);
      const std::vector<unsigned char> image = elm.saveRestart();
      FILE* o = std::fopen(argv[2], "wb");
      if (!o || std::fwrite(image.data(), 1, image.size(), o) != image.size()) throw std::runtime_error("cannot write the image");
      std::fclose(o);
      std::printf("saved %zu bytes (%.0f per column) after %d steps\n", image.size(), (double)image.size() / (double)ncols, WINDOW);
    }
    // as at start-up, but for the fields of the input file: the image brings them
    elmk::ELMInterface resumed(ncols, 0);
    start(resumed, in, NREC, NSTEPS, /*fields=*/false);
    const std::vector<char> raw = read_all(argv[2]);
    resumed.loadRestart(std::vector<unsigned char>(raw.begin(), raw.end()));
    resumed.run(dt, second);

    elmk::ELMInterface continuous(ncols, 0);
    start(continuous, in, NREC, NSTEPS);
    continuous.run(dt, steps);

    const bool same_state = resumed.saveRestart() == continuous.saveRestart();
    const auto& a = resumed.conservation();
    const auto& b = continuous.conservation();
    const bool same_cons = std::memcmp(&a, &b, sizeof a) == 0;
    std::printf("%d + %d steps with a restart vs %d continuous steps on %lld columns: %s\n", WINDOW, NSTEPS - WINDOW, NSTEPS,
                (long long)ncols, same_state && same_cons ? "bit-identical" : "DIFFERENT");
    return same_state && same_cons ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "restart_demo: %s\n", e.what());
    return 1;
  }
}
