// shortwave_demo.cc - incident shortwave from interval-mean forcing records (include/elmk.h "shortwave"), through
// include/elmk_interface.hpp: one day of 48 half-hour steps over 3-hourly FSDS records, as two runs of 24, once in each shortwave
// mode.  History tape 0 averages forc_solad and forc_solai over the day; the demo prints the domain's mean incident shortwave
// beside the records' mean.  In REFERENCE mode (the reference's ProcessFSDS) a column receives the record times the step's mean
// cos(zenith), which falls short of the records; in COSZEN mode ELM's factor spreads each record over the steps of its interval and
// the day receives what the records hold (up to the steps where cos(zenith) is at most 0.001 or the factor is capped at 10).
// The input is the flat binary file of examples/run_demo.cc with 9 three-hourly records in the atm_* series, "recs" (the record
// starts, decimal_doy + 1.0) and "steps" (48 elmk_run_step rows), written by tests/test_gpu_shortwave.py::test_shortwave_demo_runs.
//
//   g++ -std=c++17 -Iinclude examples/shortwave_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o shortwave_demo
//   ./shortwave_demo state.bin
#include <cmath>
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

static const char* const FORCING[] = {"atm_tbot", "atm_pbot", "atm_qbot", "atm_flds", "atm_fsds", "atm_prec", "atm_wind"};
static const char* const PHENOLOGY[] = {"mlai", "msai", "mhtop", "mhbot"};
constexpr int NREC = 9, NSTEPS = 48, WINDOW = 24;
constexpr double FORC_DT = 3 * 3600.0;

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin\n", argv[0]);
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

    if (sizes.at("steps") != (int64_t)(NSTEPS * sizeof(elmk_run_step))) throw std::runtime_error("steps: expected 48 rows");
    std::vector<elmk_run_step> steps(NSTEPS);
    std::memcpy(steps.data(), params.at("steps"), sizeof(elmk_run_step) * NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = D("scalars")[4];
    // the records' mean over the day: records 0 .. 7 (record 8 only brackets the last step)
    const double* fsds = D("series/atm_fsds");
    double rec_mean = 0.0;
    for (int r = 0; r < NREC - 1; r++)
      for (int64_t c = 0; c < ncols; c++) rec_mean += fsds[(size_t)r * ncols + c];
    rec_mean /= (double)(NREC - 1) * (double)ncols;

    for (const int mode : {ELMK_SW_REFERENCE, ELMK_SW_COSZEN}) {
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
      elm.set_shortwave_mode(mode, FORC_DT);
      const int solad = elm.history_add(0, "forc_solad", ELMK_HIST_AVG), solai = elm.history_add(0, "forc_solai", ELMK_HIST_AVG);
      elm.reserve_run(NREC, WINDOW);
      for (const char* f : FORCING) elm.series_upload(f, 0, NREC, D(std::string("series/") + f));
      for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
      if (mode == ELMK_SW_COSZEN) elm.series_record_times(0, NREC, D("recs"));
      elm.run(dt, first, true);
      elm.run(dt, second, true);
      std::vector<double> a((size_t)ncols * 2), b((size_t)ncols * 2);
      elm.history_read(solad, a.data());
      elm.history_read(solai, b.data());
      double day_mean = 0.0;
      for (size_t i = 0; i < a.size(); i++) day_mean += a[i] + b[i];
      day_mean /= (double)ncols;
      const double rel = day_mean / rec_mean - 1.0;
      if (mode == ELMK_SW_COSZEN)
        std::printf("coszen: %s: day's mean incident shortwave %.4f W/m2, records' mean %.4f W/m2 (%+.2e)\n",
                    std::fabs(rel) < 1e-2 ? "kept" : "NOT KEPT", day_mean, rec_mean, rel);
      else
        std::printf("reference: %s: day's mean incident shortwave %.4f W/m2, records' mean %.4f W/m2 (%+.2e)\n",
                    rel < -0.1 ? "short" : "not short", day_mean, rec_mean, rel);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shortwave_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
