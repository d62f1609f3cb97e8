// downscaling_demo.cc - forcing adjusted to column elevation (include/elmk.h "downscaling"), through include/elmk_interface.hpp:
// valley columns at the forcing cell's surface height beside mountain columns 1 500 m above it, all in one forcing cell and driven by
// the same near-freezing records, for one day of 48 half-hour steps as two runs of 24, once with downscaling OFF and once in TOPO mode
// (longwave renormalised over the cell: one group of every column, equal weights).  History tape 0 averages forc_tbot over the day;
// the demo prints the day's mean air temperature and the snow (h2osno) at the end of the day, valley beside mountain.  OFF gives every
// column the cell's air, so valley and mountain end alike; TOPO cools the mountain by the lapse rate, its precipitation falls as snow
// and the snowpack builds there.
// The input is the flat binary file of examples/run_demo.cc with 25 hourly records in the atm_* series (identical for every column),
// "topo" (each column's elevation, m), "hf" (the cell's surface height, m) and "steps" (48 elmk_run_step rows), written by
// tests/test_gpu_downscaling.py::test_downscaling_demo.
//
//   g++ -std=c++17 -Iinclude examples/downscaling_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o downscaling_demo
//   ./downscaling_demo state.bin
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
constexpr int NREC = 25, NSTEPS = 48, WINDOW = 24;

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
    const double* topo = D("topo");
    const double hf_cell = D("hf")[0];
    // every column sees the one cell's surface height; one longwave group over the cell
    const std::vector<double> hf((size_t)ncols, hf_cell), gw((size_t)ncols, 1.0 / (double)ncols);
    const std::vector<int64_t> gptr = {0, ncols};
    std::vector<int32_t> gcol((size_t)ncols);
    for (int64_t c = 0; c < ncols; c++) gcol[(size_t)c] = (int32_t)c;

    for (const int mode : {ELMK_DS_OFF, ELMK_DS_TOPO}) {
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
      elm.set_column_elevation(topo, hf.data());
      elm.set_downscaling_groups(1, gptr.data(), gcol.data(), gw.data());
      elm.set_downscaling(mode);
      const int tbot = elm.history_add(0, "forc_tbot", ELMK_HIST_AVG);
      elm.reserve_run(NREC, WINDOW);
      for (const char* f : FORCING) elm.series_upload(f, 0, NREC, D(std::string("series/") + f));
      for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
      elm.run(dt, first, true);
      elm.run(dt, second, true);
      std::vector<double> ta((size_t)ncols), sno((size_t)ncols);
      elm.history_read(tbot, ta.data());
      elm.download("h2osno", sno.data());
      double t_lo = 0.0, t_hi = 0.0, s_lo = 0.0, s_hi = 0.0;
      int64_t n_lo = 0, n_hi = 0;
      for (int64_t c = 0; c < ncols; c++) {
        if (topo[c] == hf_cell) {
          t_lo += ta[(size_t)c];
          s_lo += sno[(size_t)c];
          n_lo++;
        } else {
          t_hi += ta[(size_t)c];
          s_hi += sno[(size_t)c];
          n_hi++;
        }
      }
      if (!n_lo || !n_hi) throw std::runtime_error("need valley columns (topo == hf) and mountain columns");
      t_lo /= (double)n_lo, t_hi /= (double)n_hi, s_lo /= (double)n_lo, s_hi /= (double)n_hi;
      const char* verdict = mode == ELMK_DS_OFF ? (s_lo == s_hi && t_lo == t_hi ? "valley and mountain alike" : "NOT ALIKE")
                                                : (s_hi > s_lo && t_hi < t_lo ? "more snow on the mountain" : "NO MORE SNOW ON THE MOUNTAIN");
      std::printf("%s: %s: mean forc_tbot valley %.3f K, mountain %.3f K; h2osno valley %.3f, mountain %.3f kg/m2\n",
                  mode == ELMK_DS_OFF ? "off" : "topo", verdict, t_lo, t_hi, s_lo, s_hi);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "downscaling_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
