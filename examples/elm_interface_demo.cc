// elm_interface_demo.cc - the reference's driver loop (driver/kokkos/kokkos_driver.cc: construct ELMInterface, setup(),
// advance() per step, getPrimaryVars()) against libelmk through include/elmk_interface.hpp.
// The state and parameter arrays come from a flat binary file written by tests (tests/test_gpu_parity.py::
// test_cpp_interface_mirror): the demo has no file readers of its own, as the library has none; examples/demo_io.h describes the
// file, reads it and makes the setup() call.
//
//   g++ -std=c++17 -Iinclude examples/elm_interface_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o demo
//   ./demo state.bin nsteps out.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "demo_io.h"

int main(int argc, char** argv)
{
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s state.bin nsteps out.bin\n", argv[0]);
    return 2;
  }
  try {
    const demo::Inputs in(argv[1]);
    const int nsteps = std::atoi(argv[2]);
    const int64_t ncols = in.ncols;

    elmk::ELMInterface elm(ncols, 0);
    demo::setup(elm, in);
    demo::upload_fields(elm, in);

    elmk::StepWeights w;
    std::memcpy(w.forc_wt1, in.D("forc_wt1"), 64);
    std::memcpy(w.forc_wt2, in.D("forc_wt2"), 64);
    w.month_wt1 = in.D("month_wt")[0];
    w.month_wt2 = in.D("month_wt")[1];
    w.qbot_is_relative_humidity = 0;
    const double dt = in.dt();
    for (int s = 0; s < nsteps; s++) {
      if (elm.advance(dt, w)) return 1;
    }
    auto pv = elm.getPrimaryVars();
    FILE* o = std::fopen(argv[3], "wb");
    std::fwrite(pv->t_soisno.data(), 8, pv->t_soisno.size(), o);
    std::fwrite(pv->h2osoi_liq.data(), 8, pv->h2osoi_liq.size(), o);
    std::fwrite(pv->h2osoi_ice.data(), 8, pv->h2osoi_ice.size(), o);
    std::fwrite(pv->t_grnd.data(), 8, pv->t_grnd.size(), o);
    std::fwrite(pv->h2osno.data(), 8, pv->h2osno.size(), o);
    std::fwrite(pv->snl.data(), 4, pv->snl.size(), o);
    std::fwrite(&elm.conservation()[0][0], 8, 24, o);
    std::fclose(o);
    std::printf("advance x %d on %ld columns: ok, warning flags %#x\n", nsteps, (long)ncols, (unsigned)elm.warning_flags());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
