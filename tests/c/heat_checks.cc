// The host check of the stream temperature's inputs (elmkernels_amd/csrc/elmk_maps.h: heat_check), case by case: prints
// "<case>: <returned text>", or for accepted inputs "<case>: ok" followed, where asked for, by the KSW row of every cell as hexadecimal
// doubles.  tests/test_routing_heat_host.py compares every line with the message elmk_routing_heat_enable gives behind its own name and
// the row with routing.heat_tables, bit for bit.
#include "elmk_maps.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace elmk;

namespace {
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double Inf = std::numeric_limits<double>::infinity();

// shade of cell c: the values of valid() in turn
std::vector<double> valid(int64_t n)
{
  const double s[5] = {0.0, 1.0, 0.25, 5e-324, 0.9999999999999999};
  std::vector<double> v;
  for (int64_t c = 0; c < n; c++) v.push_back(s[c % 5]);
  return v;
}

void say(const std::string& name, int64_t n, int sublev, const double* shade, bool show = false)
{
  const int64_t ld = (n + 63) / 64 * 64;
  std::vector<double> dev;
  int64_t cell = -1;
  const char* const text = heat_check(n, sublev, shade, ld, &dev, &cell);
  if (text) {
    if (cell >= 0) printf("%s: %s at cell %lld\n", name.c_str(), text, (long long)cell);
    else printf("%s: %s\n", name.c_str(), text);
    return;
  }
  std::string s;
  if (dev.size() != (size_t)ld) s = " BAD SIZE";
  for (size_t c = (size_t)n; c < dev.size(); c++)
    if (dev[c] != 0.0) s = " BAD PADDING";
  printf("%s: ok%s", name.c_str(), s.c_str());
  if (show)
    for (int64_t c = 0; c < n; c++) printf(" %a", dev[(size_t)c]);
  printf("\n");
}
}  // namespace

int main()
{
  const int64_t n = 5;
  const std::vector<double> good = valid(n);
  say("ncells 0", 0, 0, good.data());
  say("sublev -1", n, -1, good.data());
  say("sublev 15", n, 15, good.data());
  say("sublev before shade", n, 15, nullptr);
  say("valid", n, 0, good.data(), true);
  say("sublev 14", n, 14, good.data());
  say("null shade", n, 3, nullptr, true);
  const double bads[6] = {NaN, Inf, -Inf, -1e-300, 1.0000000000000002, -5e-324};
  for (int k = 0; k < 6; k++) {
    std::vector<double> s = good;
    const int cell = k % (int)n;
    s[(size_t)cell] = bads[k];
    if (k == 5) s[4] = NaN;  // (the first offending cell is named)
    say("bad SHADE " + std::to_string(k) + " " + std::to_string(cell), n, 0, s.data());
  }
  {
    std::vector<double> s = good;
    s[2] = -0.0;  // (-0.0 >= 0.0)
    say("negative zero", n, 0, s.data(), true);
  }
  const std::vector<double> many = valid(65);
  say("sixty-five cells", 65, 7, many.data());
  {
    // ld below ncells is raised to ncells
    std::vector<double> dev;
    int64_t cell = -1;
    const char* const text = heat_check(n, 0, good.data(), 1, &dev, &cell);
    printf("short ld: %s %zu\n", text ? text : "ok", dev.size());
  }
  {
    // no table asked for, no cell asked for
    const char* const text = heat_check(n, 0, good.data(), 64, nullptr, nullptr);
    std::vector<double> s = good;
    s[3] = 2.0;
    const char* const bad = heat_check(n, 0, s.data(), 64, nullptr, nullptr);
    printf("no outputs: %s / %s\n", text ? text : "ok", bad ? bad : "ok");
  }
  return 0;
}
