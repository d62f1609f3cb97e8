// The host check of the kinematic-wave routing's parameters (elmkernels_amd/csrc/elmk_maps.h: kinematic_check), case by case: prints
// "<case>: <returned text>", or for accepted parameters "<case>: ok" followed by the seven derived rows of every cell as hexadecimal
// doubles and the state of the padding cells.  tests/test_routing_kinematic_host.py compares every line with the message
// elmk_routing_kinematic_enable gives behind its own name and the derived rows with routing.kinematic_params, bit for bit.
#include "elmk_maps.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace elmk;

namespace {
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double Inf = std::numeric_limits<double>::infinity();
const char* const NAMES[KINEMATIC_NPARAM] = {"HSLP", "NH", "GXR", "TLEN", "TWIDTH", "TSLP", "NT", "RLEN", "RWIDTH", "RSLP", "NR"};

// params [11][n]: the steady-state test's values, each scaled a little differently per cell so that no two cells share a quotient
std::vector<double> valid(int64_t n)
{
  const double base[KINEMATIC_NPARAM] = {0.05, 0.1, 1.0e-3, 1.0e5, 10.0, 0.01, 0.05, 2.0e4, 100.0, 1.0e-3, 0.04};
  std::vector<double> p((size_t)KINEMATIC_NPARAM * (size_t)n);
  for (int k = 0; k < KINEMATIC_NPARAM; k++)
    for (int64_t c = 0; c < n; c++) p[(size_t)k * (size_t)n + (size_t)c] = base[k] * (1.0 + 0.013 * (double)((c * 7 + k * 3) % 11));
  return p;
}

void say(const std::string& name, int64_t n, const double* params, bool show = false)
{
  const int64_t ld = (n + 63) / 64 * 64;
  std::vector<double> dev;
  const char* text = kinematic_check(n, params, ld, &dev);
  if (text) {
    printf("%s: %s\n", name.c_str(), text);
    return;
  }
  std::string s;
  if (dev.size() != (size_t)7 * (size_t)ld) s = " BAD SIZE";
  for (int k = 0; k < 7 && s.empty(); k++)
    for (int64_t c = n; c < ld; c++)
      if (dev[(size_t)k * (size_t)ld + (size_t)c] != 1.0) s = " BAD PADDING CELL";
  printf("%s: ok%s", name.c_str(), s.c_str());
  if (show && s.empty())
    for (int k = 0; k < 7; k++)
      for (int64_t c = 0; c < n; c++) printf(" %a", dev[(size_t)k * (size_t)ld + (size_t)c]);
  printf("\n");
}
}  // namespace

int main()
{
  const int64_t n = 5;
  const std::vector<double> good = valid(n);
  printf("ncells 0: %s\n", kinematic_check(0, good.data(), 64, nullptr));
  printf("ncells 2^31: %s\n", kinematic_check((int64_t)1 << 31, good.data(), 64, nullptr));
  printf("null params: %s\n", kinematic_check(n, nullptr, 64, nullptr));
  const double bads[] = {0.0, -0.0, -1.0, NaN, Inf, -Inf};
  const char* const bad_names[] = {"0", "-0", "negative", "NaN", "inf", "-inf"};
  for (int k = 0; k < KINEMATIC_NPARAM; k++)
    for (int b = 0; b < 6; b++) {
      std::vector<double> p = good;
      p[(size_t)k * (size_t)n + (size_t)((k + b) % n)] = bads[b];  // (first, middle and last cells in turn)
      say(std::string(NAMES[k]) + " " + bad_names[b], n, p.data());
    }
  {
    std::vector<double> p = good;  // two rows violated at once: the rows are checked in their order
    p[(size_t)9 * (size_t)n + 0] = NaN;
    p[(size_t)3 * (size_t)n + 4] = 0.0;
    say("bad RSLP and bad TLEN", n, p.data());
  }
  {
    std::vector<double> p = good;  // denormal and huge values are finite and > 0
    p[0] = 5e-324;
    p[(size_t)7 * (size_t)n + 1] = 1.7e308;
    say("denormal HSLP and huge RLEN", n, p.data());
  }
  say("valid", n, good.data(), true);
  say("one cell", 1, valid(1).data(), true);
  say("sixty-four cells", 64, valid(64).data());
  say("sixty-five cells", 65, valid(65).data());
  {
    std::vector<double> dev;  // ld below ncells: the rows are as long as the cells
    const char* text = kinematic_check(n, good.data(), 0, &dev);
    printf("ld 0: %s size=%zu\n", text ? text : "ok", dev.size());
  }
  return 0;
}
