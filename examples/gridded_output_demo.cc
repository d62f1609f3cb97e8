// gridded_output_demo.cc - history on the output grid: a day of half-hour steps with elmk_run over columns spread across the globe, and
// a history tape that averages fluxes and temperatures over the day on the cells of an output grid (include/elmk.h "output grid").
// Every step folds the area-weighted cell means of the columns (ELM's c2g) into the tape on the device; at the end of the day the
// host reads ncells values per field level instead of ncols.
// Input: the flat binary file of examples/run_demo.cc (25 hourly records, 48 steps) plus the output map ("omap/ptr" int64
// [ncells + 1], "omap/col" int32 [nnz], "omap/w" double [nnz], CSR by cell, built by elmkernels_amd/regrid.py's owner_map, and
// "omap/fill" double [1]), written by tests/test_gpu_output_grid.py::test_gridded_output_demo.
//
//   g++ -std=c++17 -Iinclude examples/gridded_output_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o gridded_output_demo
//   ./gridded_output_demo state.bin [out.bin]
//
// out.bin: the daily means of the fields of OUTPUT in that order, each [ncells][nlev] doubles.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "elmk_interface.hpp"

static std::vector<char> read_all(const char* path)
{
  FILE* f = std::fopen(path, "rb");
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> b((size_t)n);
  if (std::fread(b.data(), 1, (size_t)n, f) != (size_t)n) throw std::runtime_error("short read");
  std::fclose(f);
  return b;
}

static const char* const SERIES[] = {"atm_tbot", "atm_pbot", "atm_qbot", "atm_flds", "atm_fsds", "atm_prec", "atm_wind",
                                     "mlai",     "msai",     "mhtop",    "mhbot"};
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
    const std::vector<char> blob = read_all(argv[1]);
    const char* p = blob.data();
    const char* end = p + blob.size();
    int64_t ncols;
    std::memcpy(&ncols, p, 8);
    p += 8;
    std::map<std::string, const char*> fields, params;
    std::map<std::string, int64_t> sizes;
    while (p < end) {
      char name[33] = {0};
      std::memcpy(name, p, 32);
      int32_t kind;
      int64_t nbytes;
      std::memcpy(&kind, p + 32, 4);
      std::memcpy(&nbytes, p + 36, 8);
      (kind == 0 ? fields : params)[name] = p + 44;
      sizes[name] = nbytes;
      p += 44 + nbytes;
    }
    auto D = [&](const std::string& k) { return reinterpret_cast<const double*>(params.at(k)); };
    auto I = [&](const char* k) { return reinterpret_cast<const int32_t*>(params.at(k)); };

    elmk::ELMInterface elm(ncols, 0);
    elmk_snicar_tables t;
    std::memset(&t, 0, sizeof t);
    {
      const double** slot = reinterpret_cast<const double**>(&t);  // the struct is 31 const double* members, in this order
      for (int i = 0; i < (int)(sizeof t / sizeof(double*)); i++) slot[i] = D("snicar/" + std::to_string(i));
    }
    const int32_t* land = I("land");
    const double* sc = D("scalars");
    elm.setup(land[0], land[1], land[2], land[3], land[4], sc[0], (int)sc[1], sc[2], sc[3], D("pft_psn"), D("pft_alb"), D("z0mr"),
              D("displar"), D("albsat"), D("albdry"), &t, D("age_tau"), D("age_kappa"), D("age_drdt0"));
    for (const auto& kv : fields) elm.upload(kv.first.c_str(), kv.second);
    elm.set_column_geography(D("lat"), D("lon"));

    // the output grid: ncells from the size of ptr
    const int64_t ncells = sizes.at("omap/ptr") / (int64_t)sizeof(int64_t) - 1;
    const int64_t* ptr = reinterpret_cast<const int64_t*>(params.at("omap/ptr"));
    if (ncells < 1 || sizes.at("omap/col") != (int64_t)sizeof(int32_t) * ptr[ncells] || sizes.at("omap/w") != (int64_t)sizeof(double) * ptr[ncells])
      throw std::runtime_error("omap: expected ptr [ncells + 1], col and w [ptr[ncells]]");
    elm.set_output_grid(ncells, ptr, I("omap/col"), D("omap/w"), D("omap/fill")[0]);
    const int tape = 0;
    std::vector<int> entry, nlev;
    for (const char* f : OUTPUT) {
      entry.push_back(elm.gridded_history_add(tape, f, ELMK_HIST_AVG));
      int nl = 0;
      elmk_field_info(elmk_field_id(f), &nl, nullptr);
      nlev.push_back(nl);
    }

    if (sizes.at("steps") != (int64_t)(NSTEPS * sizeof(elmk_run_step))) throw std::runtime_error("steps: expected 48 rows");
    std::vector<elmk_run_step> steps(NSTEPS);
    std::memcpy(steps.data(), params.at("steps"), sizeof(elmk_run_step) * NSTEPS);
    const double dt = sc[4];
    elm.reserve_run(NREC, NSTEPS);
    for (const char* f : SERIES) elm.series_upload(f, 0, f[0] == 'a' ? NREC : 12, D(std::string("series/") + f));
    elm.run(dt, steps, /*accumulate_history=*/true);

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
