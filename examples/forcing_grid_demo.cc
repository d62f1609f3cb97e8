// forcing_grid_demo.cc - the driver's time loop on the device with forcing on the data set's own grid: a day of half-hour steps over
// columns spread across the globe, driven by hourly records on a 64 x 32 cell grid that the device remaps to every column
// (include/elmk.h "forcing grid").  The host sends 2048 values per record and stream instead of one per column.  48 steps run as two
// runs of 24; the cell records of the second window go up while the first run executes.
// Input: the flat binary file of examples/run_demo.cc, with the forcing as cell records ("cells/<field>": [records][ncells], 25 hourly
// records for atm_*) and the remap map ("map/idx" int32 and "map/w" double, [npts][ncols], built by elmkernels_amd/regrid.py's
// bilinear_map), written by tests/test_gpu_forcing_grid.py::test_forcing_grid_demo.
//
//   g++ -std=c++17 -Iinclude examples/forcing_grid_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o forcing_grid_demo
//   ./forcing_grid_demo state.bin [out.bin]
//
// out.bin: as run_demo's - the PrimaryVars members in ELMInterface order, then the 48 conservation rows [48][8][3] doubles.
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

    // the map: npts rows of ncols terms; ncells from the size of a cell record
    const int npts = (int)(sizes.at("map/idx") / (int64_t)(sizeof(int32_t) * ncols));
    if (sizes.at("map/w") != (int64_t)(sizeof(double)) * npts * ncols) throw std::runtime_error("map/w: expected [npts][ncols]");
    const int64_t ncells = sizes.at("cells/atm_tbot") / (int64_t)(sizeof(double) * NREC);
    elm.set_forcing_grid(ncells, npts, I("map/idx"), D("map/w"));

    if (sizes.at("steps") != (int64_t)(NSTEPS * sizeof(elmk_run_step))) throw std::runtime_error("steps: expected 48 rows");
    std::vector<elmk_run_step> steps(NSTEPS);
    std::memcpy(steps.data(), params.at("steps"), sizeof(elmk_run_step) * NSTEPS);
    const std::vector<elmk_run_step> first(steps.begin(), steps.begin() + WINDOW), second(steps.begin() + WINDOW, steps.end());
    const double dt = sc[4];

    // 25 cell records per forcing stream and the 12 months (per column) on the device; the first window's records (slots 0 .. 12)
    // before the first run.  The reservation comes after set_forcing_grid: it sizes the forcing series by cells.
    elm.reserve_run(NREC, WINDOW);
    const int split = first.back().forc_slot + 2;  // records the first run reads: 0 .. split - 1
    for (const char* f : FORCING) elm.series_upload_cells(f, 0, split, D(std::string("cells/") + f));
    for (const char* f : PHENOLOGY) elm.series_upload(f, 0, 12, D(std::string("series/") + f));
    elm.enqueue_run(dt, first);
    // the second window goes up while the first run executes (it reads none of these records, so nothing waits)
    for (const char* f : FORCING) elm.series_upload_cells(f, split, NREC - split, D(std::string("cells/") + f) + (size_t)split * ncells);
    elm.finish_run();
    std::vector<double> cons = elm.run_conservation();
    elm.run(dt, second);
    cons.insert(cons.end(), elm.run_conservation().begin(), elm.run_conservation().end());

    const auto pv = elm.getPrimaryVars();
    std::printf("%d steps on %lld columns from %lld forcing cells (%d terms per column) in two runs: water balance error of the last "
                "step %.3e .. %.3e kg/m2\n", NSTEPS, (long long)ncols, (long long)ncells, npts, elm.conservation()[1][0],
                elm.conservation()[1][1]);
    if (argc > 2) {
      FILE* o = std::fopen(argv[2], "wb");
      if (!o) throw std::runtime_error(std::string("cannot open ") + argv[2]);
      put(o, pv->snl);
      put(o, pv->snow_depth);
      put(o, pv->frac_sno);
      put(o, pv->int_snow);
      put(o, pv->snw_rds);
      put(o, pv->h2osoi_liq);
      put(o, pv->h2osoi_ice);
      put(o, pv->h2osoi_vol);
      put(o, pv->h2ocan);
      put(o, pv->h2osno);
      put(o, pv->h2osfc);
      put(o, pv->t_soisno);
      put(o, pv->t_grnd);
      put(o, pv->t_h2osfc);
      put(o, pv->t_h2osfc_bef);
      put(o, pv->nrad);
      put(o, pv->dz);
      put(o, pv->zsoi);
      put(o, pv->zisoi);
      put(o, cons);
      std::fclose(o);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "forcing_grid_demo: %s\n", e.what());
    return 1;
  }
  return 0;
}
