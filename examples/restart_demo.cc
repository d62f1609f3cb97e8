// restart_demo.cc - an exact restart (E3SM's ERS test) through include/elmk_interface.hpp: 24 half-hour steps, saveRestart() to a
// file, the context destroyed; a new context set up as at start-up, loadRestart() from the file, 24 more steps.  The result is set
// against one continuous run of 48 steps and the demo prints whether the two are bit-identical (their restart images and the last
// step's conservation diagnostics).  Input: the state.bin of examples/run_demo.cc (written by tests/test_gpu_run.py::test_run_demo,
// and by tests/test_gpu_restart.py::test_restart_demo).
//
//   g++ -std=c++17 -Iinclude examples/restart_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o restart_demo
//   ./restart_demo state.bin restart.img
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
constexpr int NREC = 25, NSTEPS = 48, WINDOW = 24;

struct Inputs {
  int64_t ncols;
  std::map<std::string, const char*> fields, params;
  std::map<std::string, int64_t> sizes;
};

// start-up: parameters and tables, the fields of the input file (skipped when a restart image follows), geography, the run series
static void start(elmk::ELMInterface& elm, Inputs& in, bool upload_fields)
{
  auto D = [&](const std::string& k) { return reinterpret_cast<const double*>(in.params.at(k)); };
  auto I = [&](const char* k) { return reinterpret_cast<const int32_t*>(in.params.at(k)); };
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
  if (upload_fields)
    for (const auto& kv : in.fields) elm.upload(kv.first.c_str(), kv.second);
  elm.set_column_geography(D("lat"), D("lon"));
  elm.reserve_run(NREC, NSTEPS);
  for (const char* f : FORCING) elm.series_upload(f, 0, NREC, D(std::string("series/") + f));
  for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
}

int main(int argc, char** argv)
{
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s state.bin restart.img\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<char> blob = read_all(argv[1]);
    const char* p = blob.data();
    const char* end = p + blob.size();
    int64_t ncols;
    std::memcpy(&ncols, p, 8);
    p += 8;
    Inputs in;
    std::map<std::string, const char*>& fields = in.fields;
    std::map<std::string, const char*>& params = in.params;
    std::map<std::string, int64_t>& sizes = in.sizes;
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

    in.ncols = ncols;
    if (sizes.at("steps") != (int64_t)(NSTEPS * sizeof(elmk_run_step))) throw std::runtime_error("steps: expected 48 rows");
    std::vector<elmk_run_step> steps(NSTEPS);
    std::memcpy(steps.data(), params.at("steps"), sizeof(elmk_run_step) * NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = reinterpret_cast<const double*>(params.at("scalars"))[4];

    {  // the first half, saved to a file; the context ends with the scope
      elmk::ELMInterface elm(ncols, 0);
      start(elm, in, true);
      elm.run(dt, first);
      const std::vector<unsigned char> image = elm.saveRestart();
      FILE* o = std::fopen(argv[2], "wb");
      if (!o || std::fwrite(image.data(), 1, image.size(), o) != image.size()) throw std::runtime_error("cannot write the image");
      std::fclose(o);
      std::printf("saved %zu bytes (%.0f per column) after %d steps\n", image.size(), (double)image.size() / (double)ncols, WINDOW);
    }
    elmk::ELMInterface resumed(ncols, 0);
    start(resumed, in, false);
    const std::vector<char> raw = read_all(argv[2]);
    resumed.loadRestart(std::vector<unsigned char>(raw.begin(), raw.end()));
    resumed.run(dt, second);

    elmk::ELMInterface continuous(ncols, 0);
    start(continuous, in, true);
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
