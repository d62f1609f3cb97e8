// The host check of elmk_hillslope_enable (elmkernels_amd/csrc/elmk_maps.h: hillslope_check; include/elmk.h "hillslope lateral flow"),
// case by case: prints "<case>: <text> @<col>" for a refusal, the text of the first failing check and the first offending column (-1
// where the text is about no column), or "<case>: ok nup=<largest in-degree> up=<the uphill map, row by row, rows joined by |>" for
// an accepted set (a long map prints its size and a sum instead).  tests/test_hillslope_host.py compares every line with
// hydrology.hillslope_check and hydrology.hillslope_map.
#include "elmk_maps.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace elmk;

namespace {
struct Set {
  std::vector<int32_t> down;
  std::vector<double> dist, width, area, elev;
  double k = 10.0;
  explicit Set(std::vector<int32_t> d) : down(std::move(d)), dist(down.size(), 50.0), width(down.size(), 30.0), area(down.size(), 1500.0), elev(down.size(), 2.0) {}
};

void say(const char* name, const Set& s, bool show = true, bool null_elev = false)
{
  int nup = -7;
  int64_t col = -7;
  std::vector<int32_t> up{7, 7, 7};  // (what it held goes, or stays untouched under a refusal)
  const int64_t n = (int64_t)s.down.size();
  const char* text = hillslope_check(n, s.down.data(), s.dist.data(), s.width.data(), s.area.data(), null_elev ? nullptr : s.elev.data(), s.k, n,
                                     &nup, &up, &col);
  if (text) {
    printf("%s: %s @%lld%s\n", name, text, (long long)col, (up.size() != 3 || up[0] != 7 || nup != -7) ? " (outputs written)" : "");
    return;
  }
  printf("%s: ok nup=%d up=", name, nup);
  if (show) {
    for (size_t i = 0; i < up.size(); i++) printf("%s%d", i == 0 ? "" : (i % (size_t)n == 0 ? "|" : " "), up[i]);
  } else {
    long long sum = 0, none = 0;
    for (int32_t u : up) sum += u, none += u < 0;
    printf("size=%zu sum=%lld none=%lld", up.size(), sum, none);
  }
  printf("\n");
}
}  // namespace

int main()
{
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  say("one column to the stream", Set({-1}));
  say("one column on no hillslope", Set({-2}));
  say("a chain of five", Set({-1, 0, 1, 2, 3}));
  for (int k = 0; k <= 8; k++) {  // in-degrees 0 .. 8: column 0 at the stream under k uphill columns, a -2 column behind them
    std::vector<int32_t> d(1, -1);
    for (int i = 0; i < k; i++) d.push_back(0);
    d.push_back(-2);
    char name[32];
    snprintf(name, sizeof name, "in-degree %d", k);
    say(name, Set(d));
  }
  say("slots ascend whatever the order", Set({3, 3, -1, 2, 3, 2}));
  say("null argument", Set({-1}), true, true);
  say("down below -2", Set({-1, -3, 0}));
  say("down past the columns", Set({-1, 3, 0}));
  say("self-loop", Set({-1, 0, 2}));
  say("range before self-loop", Set({0, 9}));
  say("into a column on no hillslope", Set({-2, 0, -1}));
  say("self-loop before a -2 target", Set({-2, 0, 2}));
  say("nine uphill columns", Set({-1, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
  say("a cycle of two", Set({-1, 2, 1}));
  say("a cycle behind a tail", Set({1, 2, 3, 1, -1}));
  say("in-degree before a cycle", Set({1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}));
  {
    Set s({-1, 0, -2});
    s.dist[1] = 0.0;
    s.width[0] = nan;
    say("dist before width", s);
    s.dist[1] = 50.0;
    say("width NaN", s);
    s.width[0] = 30.0;
    s.area[1] = -1.0;
    say("area negative", s);
    s.area[1] = inf;
    say("area infinite", s);
    s.area[1] = 1500.0;
    s.elev[0] = inf;
    say("elev infinite", s);
    s.elev[0] = -3.0;
    s.dist[2] = nan, s.width[2] = 0.0, s.area[2] = -inf, s.elev[2] = nan;
    say("nothing is asked of a column on no hillslope", s);
    s.k = 0.0;
    say("k_aniso zero", s);
    s.k = nan;
    say("k_aniso NaN", s);
    s.k = inf;
    say("k_aniso infinite", s);
  }
  // a long chain: 200 000 columns, each draining into the one before it (nothing recurses), then closed into a cycle
  std::vector<int32_t> d(200000);
  for (size_t i = 0; i < d.size(); i++) d[i] = (int32_t)i - 1;
  say("a chain of 200000", Set(d), false);
  d[0] = (int32_t)d.size() - 1;
  say("... closed into a cycle", Set(d), false);
  return 0;
}
