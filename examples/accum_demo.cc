// accum_demo.cc - ELM's T10 kept on the device (elmk.h "accumulated fields") through include/elmk_interface.hpp: 48 half-hour steps
// as ONE run whose every step folds t_ref2m into a running mean over 8 steps and writes it to t10, the field photosynthesis reads
// for its acclimation terms.  The result is set against the loop this replaces - one run per step, and between two steps the host
// downloads t_ref2m, applies the update and uploads t10 - and against a run that leaves t10 at its start-up value.  The demo prints
// whether the first two are bit-identical (restart images, the accumulator and its step count) and how far t10 has moved.  Input:
// the state.bin of examples/run_demo.cc (written by tests/test_gpu_run.py::test_run_demo and tests/test_gpu_accum.py::test_accum_demo).
//
//   g++ -std=c++17 -Iinclude examples/accum_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o accum_demo
//   ./accum_demo state.bin
#include <algorithm>
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
constexpr int NREC = 25, NSTEPS = 48;
constexpr int64_t PERIOD = 8;  // steps of the running mean (ELM: ten days)

struct Inputs {
  int64_t ncols;
  std::map<std::string, const char*> fields, params;
  std::map<std::string, int64_t> sizes;
};

// start-up: parameters and tables, the fields of the input file, geography, the run series
static void start(elmk::ELMInterface& elm, Inputs& in)
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
  for (const auto& kv : in.fields) elm.upload(kv.first.c_str(), kv.second);
  elm.set_column_geography(D("lat"), D("lon"));
  elm.reserve_run(NREC, NSTEPS);
  for (const char* f : FORCING) elm.series_upload(f, 0, NREC, D(std::string("series/") + f));
  for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
}

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
    Inputs in;
    in.ncols = ncols;
    while (p < end) {
      char name[33] = {0};
      std::memcpy(name, p, 32);
      int32_t kind;
      int64_t nbytes;
      std::memcpy(&kind, p + 32, 4);
      std::memcpy(&nbytes, p + 36, 8);
      (kind == 0 ? in.fields : in.params)[name] = p + 44;
      in.sizes[name] = nbytes;
      p += 44 + nbytes;
    }

    if (in.sizes.at("steps") != (int64_t)(NSTEPS * sizeof(elmk_run_step))) throw std::runtime_error("steps: expected 48 rows");
    std::vector<elmk_run_step> steps(NSTEPS);
    std::memcpy(steps.data(), in.params.at("steps"), sizeof(elmk_run_step) * NSTEPS);
    const double dt = reinterpret_cast<const double*>(in.params.at("scalars"))[4];
    const size_t n = (size_t)ncols;

    // on the device: the value starts from the t10 that was uploaded, as a window that is already full
    elmk::ELMInterface device(ncols, 0);
    start(device, in);
    const int entry = device.accum_add("t_ref2m", ELMK_ACCUM_RUNMEAN, PERIOD, "t10");
    device.accum_init(entry, nullptr, PERIOD);
    device.run(dt, steps, false, false, true);
    std::vector<double> val(n);
    const int64_t count = device.accum_read(entry, val.data());

    // the loop it replaces: a round trip through the host after every step
    elmk::ELMInterface host(ncols, 0);
    start(host, in);
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
    start(frozen, in);
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
