// aerosol_demo.cc - aerosol deposition from a monthly climatology kept on the device (elmk.h "aerosol deposition") through
// include/elmk_interface.hpp: the twelve months of the eleven deposition streams live on the aerosol file's own grid (here ELM's
// 1.9 x 2.5 degree grid, 144 x 96 cells, filled with a synthetic seasonal cycle), every column picks its nearest cell, and 48
// half-hour steps run as ONE elmk_run whose every step interpolates aer_* between the step's two months - the schedule crosses from
// the bracket (December, January) to (January, February) half way.  The result is set against the loop this replaces, one
// update_aerosol() and one one-step run per step, and against a run that leaves aer_* at their start-up values.  The demo prints
// mss_dst1 of a snow-covered column after each and exits non-zero unless the first two are bit-identical.  Input: the state.bin of
// examples/run_demo.cc (written by tests/test_gpu_run.py::test_run_demo and tests/test_gpu_aerosol.py::test_aerosol_demo);
// examples/demo_io.h reads it and starts a context up.
//
//   g++ -std=c++17 -Iinclude examples/aerosol_demo.cc -Lelmkernels_amd -lelmk -Wl,-rpath,$PWD/elmkernels_amd -o aerosol_demo
//   ./aerosol_demo state.bin
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "demo_io.h"

static const char* const STREAMS[] = {"aer_bcphi",  "aer_bcpho",  "aer_bcdep",  "aer_dst1_1", "aer_dst1_2", "aer_dst2_1",
                                      "aer_dst2_2", "aer_dst3_1", "aer_dst3_2", "aer_dst4_1", "aer_dst4_2"};
constexpr int NREC = 25, NSTEPS = 48, NSTREAM = 11, NMONTH = 12;
constexpr int NLON = 144, NLAT = 96;  // the aerosol file's grid: cell = j * NLON + i, j from the south, i eastwards from 0 degrees
constexpr int64_t NCELLS = (int64_t)NLON * NLAT;
constexpr double PI = 3.14159265358979323846;

// the nearest-cell pick of the reference's aerosol reader (aerosol_data_old_impl.hh:32-55): one term of weight 1 per column
static void nearest_map(const double* lat_r, const double* lon_r, int64_t n, std::vector<int32_t>& idx, std::vector<double>& w)
{
  idx.resize((size_t)n);
  w.assign((size_t)n, 1.0);
  for (int64_t c = 0; c < n; c++) {
    double x = std::fmod(lon_r[c] * 180.0 / PI, 360.0);
    if (x < 0.0) x += 360.0;
    const int i = std::min(NLON - 1, (int)std::floor(x / (360.0 / NLON)));
    const double y = std::min(90.0, std::max(-90.0, lat_r[c] * 180.0 / PI));
    const int j = std::min(NLAT - 1, std::max(0, (int)std::floor((y + 90.0) / (180.0 / NLAT))));
    idx[(size_t)c] = j * NLON + i;
  }
}

// a synthetic climatology [NSTREAM][NMONTH][NCELLS], kg/m2/s: dust peaks in April and comes from a belt around 30 N, black carbon
// has a weak winter maximum
static std::vector<double> climatology()
{
  std::vector<double> x((size_t)NSTREAM * NMONTH * NCELLS);
  for (int s = 0; s < NSTREAM; s++)
    for (int m = 0; m < NMONTH; m++) {
      const double spring = 0.5 * (1.0 + std::cos(2.0 * PI * (m - 3) / 12.0)), winter = 0.5 * (1.0 + std::cos(2.0 * PI * m / 12.0));
      const bool bc = s < 3;
      const double amp = bc ? 2.0e-13 * (1.0 + 0.3 * s) * (0.7 + 0.3 * winter) : 5.0e-11 * (1.0 + 0.2 * s) * (0.05 + 0.95 * spring * spring);
      for (int j = 0; j < NLAT; j++) {
        const double lat = -90.0 + (j + 0.5) * 180.0 / NLAT;
        const double belt = std::exp(-(lat - 30.0) * (lat - 30.0) / 800.0);
        for (int i = 0; i < NLON; i++)
          x[((size_t)s * NMONTH + m) * NCELLS + (size_t)j * NLON + i] = amp * (0.1 + belt) * (1.0 + 0.5 * std::sin(0.1 * i + s));
      }
    }
  return x;
}

// start-up as every run demo's, then the aerosol series and map
static void start(elmk::ELMInterface& elm, const demo::Inputs& in, const std::vector<double>& clim)
{
  demo::start(elm, in, NREC, NSTEPS);
  std::vector<int32_t> idx;
  std::vector<double> w;
  nearest_map(in.D("lat"), in.D("lon"), in.ncols, idx, w);
  elm.aerosol_reserve(NCELLS, 1, idx.data(), w.data());
  for (int s = 0; s < NSTREAM; s++) elm.aerosol_upload(STREAMS[s], 0, NMONTH, clim.data() + (size_t)s * NMONTH * NCELLS);
}

int main(int argc, char** argv)
{
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s state.bin\n", argv[0]);
    return 2;
  }
  try {
    const demo::Inputs in(argv[1]);
    const int64_t ncols = in.ncols;
    const std::vector<elmk_run_step> steps = demo::run_steps(in, NSTEPS);
    if (steps.front().month1 == steps.back().month1) throw std::runtime_error("steps: the schedule stays inside one month bracket");
    const double dt = in.dt();
    const size_t n = (size_t)ncols;
    const std::vector<double> clim = climatology();

    // on the device: every step of one run interpolates the eleven streams
    elmk::ELMInterface device(ncols, 0);
    start(device, in, clim);
    device.run(dt, steps, false, false, false, true);

    // the loop it replaces: one call per step from the host, with that step's bracket
    elmk::ELMInterface loop(ncols, 0);
    start(loop, in, clim);
    for (int s = 0; s < NSTEPS; s++) {
      const elmk_run_step& q = steps[(size_t)s];
      loop.update_aerosol(q.month1, q.month2, q.month_wt1, q.month_wt2);
      loop.run(dt, std::vector<elmk_run_step>(1, q));
    }

    // and aer_* left alone: deposition frozen at what was uploaded
    elmk::ELMInterface frozen(ncols, 0);
    start(frozen, in, clim);
    frozen.run(dt, steps);

    const bool same_state = device.saveRestart() == loop.saveRestart();
    std::vector<int32_t> snl(n);
    std::vector<double> a(n * 5), b(n * 5), f(n * 5);
    device.download("snl", snl.data());
    device.download("mss_dst1", a.data());
    loop.download("mss_dst1", b.data());
    frozen.download("mss_dst1", f.data());
    int64_t col = -1, moved = 0;
    for (size_t c = 0; c < n; c++) {
      if (snl[c] <= 0) continue;
      if (col < 0) col = (int64_t)c;
      moved += std::memcmp(&a[c * 5], &f[c * 5], 5 * sizeof(double)) != 0;
    }
    if (col < 0) throw std::runtime_error("no column with a snow layer");
    const size_t top = (size_t)col * 5 + (size_t)(5 - snl[(size_t)col]);  // the top snow layer receives the deposition
    std::printf("aerosol deposition from %lld cells, %d steps on %lld columns: run vs stepwise loop %s\n", (long long)NCELLS, NSTEPS,
                (long long)ncols, same_state ? "bit-identical" : "DIFFERENT");
    std::printf("mss_dst1 of column %lld (snl %d), top layer: run %.17g  loop %.17g  frozen aer_* %.17g; %lld snow columns differ from frozen\n",
                (long long)col, (int)snl[(size_t)col], a[top], b[top], f[top], (long long)moved);
    return same_state && a[top] == b[top] && moved > 0 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "aerosol_demo: %s\n", e.what());
    return 1;
  }
}
