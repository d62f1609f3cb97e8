// active_layer_demo.cc - ELM's active layer thickness kept on the device (elmk.h "active layer thickness") through
// include/elmk_interface.hpp: a short run of half-hour steps across 00:00 of 1 January as ONE run whose every step computes the depth
// of the thaw front from t_soisno, keeps the annual maximum and, on the step that starts the new year, rolls the maximum of the
// northern columns over into last year's.  The result is set against the loop this replaces - one run per step and a stepwise
// update_active_layer() with the rollover bits the driver derives from the date - and the three rows ALT, ALTMAX and ALTMAX_LASTYEAR
// of a few columns are printed with the two layer indices.  Input: the state.bin of examples/run_demo.cc with a schedule that crosses
// the new year (written by tests/test_gpu_active_layer.py::test_active_layer_demo).
//
//   g++ -std=c++17 -Iinclude examples/active_layer_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o active_layer_demo
//   ./active_layer_demo state.bin
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
constexpr int NREC = 25;

struct Inputs {
  int64_t ncols;
  std::map<std::string, const char*> fields, params;
  std::map<std::string, int64_t> sizes;
};

// start-up: parameters and tables, the fields of the input file, geography, the run series; a cold start of the feature
static void start(elmk::ELMInterface& elm, Inputs& in, int nsteps)
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
  elm.reserve_run(NREC, nsteps);
  for (const char* f : FORCING) elm.series_upload(f, 0, NREC, D(std::string("series/") + f));
  for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
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
    const int nsteps = (int)(in.sizes.at("steps") / (int64_t)sizeof(elmk_run_step));
    if (nsteps < 1 || in.sizes.at("steps") != (int64_t)(nsteps * sizeof(elmk_run_step))) throw std::runtime_error("steps: not whole rows");
    std::vector<elmk_run_step> steps((size_t)nsteps);
    std::memcpy(steps.data(), in.params.at("steps"), sizeof(elmk_run_step) * (size_t)nsteps);
    const double dt = reinterpret_cast<const double*>(in.params.at("scalars"))[4];
    const double* lat = reinterpret_cast<const double*>(in.params.at("lat"));
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
