// gridded_output_demo.cc - history on the output grid: a day of half-hour steps with elmk_run over columns spread across the globe, and
// a history tape that averages fluxes and temperatures over the day on the cells of an output grid (include/elmk.h "output grid").
// Every step folds the area-weighted cell means of the columns (ELM's c2g) into the tape on the device; at the end of the day the
// host reads ncells values per field level instead of ncols.
// Input: the flat binary file of examples/run_demo.cc (25 hourly records, 48 steps) plus the output map ("omap/ptr" int64
// [ncells + 1], "omap/col" int32 [nnz], "omap/w" double [nnz], CSR by cell, built by elmkernels_amd/regrid.py's owner_map, and
// "omap/fill" double [1]), written by tests/test_gpu_output_grid.py::test_gridded_output_demo; examples/demo_io.h reads it.
//
//   g++ -std=c++17 -Iinclude examples/gridded_output_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o gridded_output_demo
//   ./gridded_output_demo state.bin [out.bin]
//
// out.bin: the daily means of the fields of OUTPUT in that order, each [ncells][nlev] doubles.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "demo_io.h"

using namespace demo;
// the tape: daily means on the cells (t_soisno: every level)
static const char* const OUTPUT[] = {"eflx_sh_tot", "eflx_lh_tot", "qflx_evap_tot", "fsa", "eflx_lwrad_out", "t_grnd", "t_soisno"};
constexpr int NREC = 25, NSTEPS = 48;

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

    // the output grid: ncells from the size of ptr
    const int64_t ncells = in.sizes.at("omap/ptr") / (int64_t)sizeof(int64_t) - 1;
    const int64_t* ptr = reinterpret_cast<const int64_t*>(in.params.at("omap/ptr"));
    if (ncells < 1 || in.sizes.at("omap/col") != (int64_t)sizeof(int32_t) * ptr[ncells] ||
        in.sizes.at("omap/w") != (int64_t)sizeof(double) * ptr[ncells])
      throw std::runtime_error("omap: expected ptr [ncells + 1], col and w [ptr[ncells]]");
    elm.set_output_grid(ncells, ptr, in.I("omap/col"), in.D("omap/w"), in.D("omap/fill")[0]);
    const int tape = 0;
    std::vector<int> entry, nlev;
    for (const char* f : OUTPUT) {
      entry.push_back(elm.gridded_history_add(tape, f, ELMK_HIST_AVG));
      int nl = 0;
      elmk_field_info(elmk_field_id(f), &nl, nullptr);
      nlev.push_back(nl);
    }

    const std::vector<elmk_run_step> steps = run_steps(in, NSTEPS);
    elm.reserve_run(NREC, NSTEPS);
    upload_series(elm, in, NREC);
    elm.run(in.dt(), steps, /*accumulate_history=*/true);

    std::vector<std::vector<double>> mean(entry.size());
    for (size_t k = 0; k < entry.size(); k++) {
      mean[k].resize((size_t)ncells * (size_t)nlev[k]);
      elm.gridded_history_read(entry[k], mean[k].data());
    }
    double lo = 1e300, hi = -1e300;
    for (int64_t i = 0; i < ncells; i++)  // (cells without columns read the fill value)
      if (ptr[i + 1] > ptr[i]) lo = std::min(lo, mean[5][(size_t)i]), hi = std::max(hi, mean[5][(size_t)i]);
    std::printf("%lld samples on %lld columns: daily means of %d fields on %lld cells (%lld map terms); t_grnd %.2f .. %.2f K\n",
                (long long)elm.history_count(tape), (long long)ncols, (int)entry.size(), (long long)ncells, (long long)ptr[ncells], lo, hi);
    if (argc > 2) {
      FILE* o = std::fopen(argv[2], "wb");
      if (!o) throw std::runtime_error(std::string("cannot open ") + argv[2]);
      for (const auto& m : mean) put(o, m);
      std::fclose(o);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "gridded_output_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
