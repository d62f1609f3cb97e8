// The host check of the river network (elmkernels_amd/csrc/elmk_maps.h: route_check), case by case: prints "<case>: <returned text>",
// or "<case>: ok nup=<largest in-degree> npad=<rows of the map> up=<the map's entries of cell 0 ..>" for an accepted network.
// tests/test_routing_host.py compares every line with the message elmk_routing_enable gives behind its own name.
#include "elmk_maps.h"

#include <cstdio>
#include <limits>
#include <string>
#include <vector>

using namespace elmk;

namespace {
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double Inf = std::numeric_limits<double>::infinity();

struct Net {
  std::vector<int32_t> down;
  std::vector<double> ddist, area;
  explicit Net(std::vector<int32_t> d) : down(std::move(d)), ddist(down.size(), 1000.0), area(down.size(), 1.0e6) {}
  int64_t n() const { return (int64_t)down.size(); }
};

// show: the cells whose upstream slots are printed after an accepted network
void say(const char* name, const Net& N, const std::vector<int64_t>& show = {})
{
  int nup = -1;
  std::vector<int32_t> up;
  const int64_t ld = (N.n() + 63) / 64 * 64;
  const char* text = route_check(N.n(), N.down.data(), N.ddist.data(), N.area.data(), ld, &nup, &up);
  if (text) {
    printf("%s: %s\n", name, text);
    return;
  }
  const int npad = ell_npad(nup);
  std::string s;
  if (up.size() != (size_t)npad * (size_t)ld) s = " BAD MAP SIZE";
  // every slot against the definition: the p-th u with down[u] == c in ascending u (quadratic: small networks only)
  if (N.n() <= 4096) {
    for (int64_t c = 0; c < N.n(); c++) {
      int p = 0;
      for (int64_t u = 0; u < N.n(); u++)
        if (N.down[(size_t)u] == c) {
          if (p >= npad || up[(size_t)p * ld + c] != u) s = " BAD SLOT";
          p++;
        }
      for (; p < npad; p++)
        if (up[(size_t)p * ld + c] != -1) s = " BAD PADDING";
    }
    for (int p = 0; p < npad; p++)
      for (int64_t c = N.n(); c < ld; c++)
        if (up[(size_t)p * ld + c] != -1) s = " BAD PADDING CELL";
  }
  for (int64_t c : show) {
    s += " " + std::to_string(c) + ":";
    for (int p = 0; p < npad; p++) s += (p ? "," : "") + std::to_string(up[(size_t)p * ld + c]);
  }
  printf("%s: ok nup=%d npad=%d%s\n", name, nup, npad, s.c_str());
}

Net chain(int64_t n, bool reverse)
{
  std::vector<int32_t> d((size_t)n);
  for (int64_t c = 0; c < n; c++) d[(size_t)c] = reverse ? (int32_t)(c - 1) : (c + 1 < n ? (int32_t)(c + 1) : -1);
  return Net(d);
}

// `k` cells draining into cell 0 of k + 1
Net star(int k)
{
  std::vector<int32_t> d((size_t)k + 1, 0);
  d[0] = -1;
  return Net(d);
}
}  // namespace

int main()
{
  const Net small({1, 2, -1, 2});
  {
    int nup;
    std::vector<int32_t> up;
    printf("ncells 0: %s\n", route_check(0, small.down.data(), small.ddist.data(), small.area.data(), 64, &nup, &up));
    printf("ncells 2^31: %s\n", route_check((int64_t)1 << 31, small.down.data(), small.ddist.data(), small.area.data(), 64, &nup, &up));
    printf("null down: %s\n", route_check(4, nullptr, small.ddist.data(), small.area.data(), 64, &nup, &up));
    printf("null ddist: %s\n", route_check(4, small.down.data(), nullptr, small.area.data(), 64, &nup, &up));
    printf("null area: %s\n", route_check(4, small.down.data(), small.ddist.data(), nullptr, 64, &nup, &up));
  }
  say("down -2", Net({1, -2, -1, 2}));
  say("down ncells", Net({1, 4, -1, 2}));
  say("down == self", Net({1, 2, -1, 3}));
  say("2-cycle", Net({1, 0, -1, 2}));
  say("cycle of all cells", Net({1, 2, 3, 0}));
  say("cycle reached from a tail", Net({1, 2, 3, 4, 2, -1}));
  say("cycle reached from two tails, the second after it is marked", Net({3, 3, 4, 4, 5, 3, 0}));
  say("nine upstream cells", star(9));
  {
    Net n = small;
    n.ddist[1] = 0.0;
    say("ddist 0", n);
    n.ddist[1] = -1.0;
    say("ddist negative", n);
    n.ddist[1] = NaN;
    say("ddist NaN", n);
    n.ddist[1] = Inf;
    say("ddist inf", n);
    n = small;
    n.area[3] = -1.0;
    say("area negative", n);
    n.area[3] = NaN;
    say("area NaN", n);
    n.area[3] = Inf;
    say("area inf", n);
    n.area[3] = 0.0;
    say("area 0", n);
    n.ddist[0] = NaN;  // two checks violated at once: the network's come before ddist, ddist before area
    n.area[0] = NaN;
    say("bad ddist and bad area", n);
    n.down[0] = 0;
    say("self-loop with a bad ddist", n);
  }
  say("valid small", small, {0, 1, 2, 3});
  say("exactly eight upstream cells", star(8), {0, 1});
  say("five upstream cells", star(5), {0});
  say("all cells outlets", Net(std::vector<int32_t>(100, -1)), {0, 99});
  say("one cell", Net({-1}), {0});
  say("two trees joining downstream of a visited path", Net({2, 2, 5, 4, 5, -1}), {2, 5});
  say("chain of 100000 cells", chain(100000, false), {0, 1, 99999});
  say("reverse chain of 100000 cells", chain(100000, true), {0, 99998, 99999});
  return 0;
}
