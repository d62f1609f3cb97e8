// The column-uniqueness check of elmk_irrigation_supply_enable (elmkernels_amd/csrc/elmk_maps.h: csr_shared_column), case by case:
// prints "<case>: <returned value>" - the first column an earlier term holds already, -1 for a map with every column in at most one
// cell, -2 for a column out of range before any repeat.  And csr_check's own answers on the same maps, since both run one scan.
// tests/test_irrigation_supply_host.py compares every line.
#include "elmk_maps.h"

#include <cstdio>
#include <vector>

using namespace elmk;

namespace {
void say(const char* name, int64_t ncols, const std::vector<int32_t>& col)
{
  printf("%s: %lld\n", name, (long long)csr_shared_column(ncols, (int64_t)col.size(), col.empty() ? nullptr : col.data()));
}
}  // namespace

int main()
{
  say("no terms", 5, {});
  say("one term", 5, {4});
  say("every column once", 5, {3, 0, 4, 1, 2});
  say("columns in no cell", 9, {8, 0});
  say("last column twice", 5, {0, 4, 1, 4});
  say("first column twice, adjacent", 5, {0, 0, 1});
  say("two repeats, the first in term order wins", 6, {5, 2, 3, 2, 5, 3});
  say("three times", 4, {1, 1, 1});
  say("column out of range before a repeat", 4, {0, 4, 0});
  say("column negative before a repeat", 4, {0, -1, 0});
  say("repeat before a column out of range", 4, {0, 0, 9});
  say("no columns at all", 0, {});
  // a long map: 100 000 columns once each in reverse order, then column 77 again as the last term
  std::vector<int32_t> big(100000);
  for (size_t i = 0; i < big.size(); i++) big[i] = (int32_t)(big.size() - 1 - i);
  say("100000 columns once", 100000, big);
  big.push_back(77);
  say("100000 columns and one again", 100000, big);
  // csr_check gives what it gave: the scan is shared
  const int64_t ptr[4] = {0, 1, 2, 3};
  const int32_t rep[3] = {2, 0, 2}, fine[3] = {2, 0, 1};
  const double w[3] = {1.0, 0.5, 0.25};
  const char* t = csr_check(3, 3, ptr, rep, w, "bad", true, true);
  printf("csr_check unique on a repeat: %s\n", t ? t : "ok");
  t = csr_check(3, 3, ptr, rep, w, "bad", false, false);
  printf("csr_check repeats allowed: %s\n", t ? t : "ok");
  t = csr_check(3, 3, ptr, fine, w, "bad", true, true);
  printf("csr_check unique, no repeat: %s\n", t ? t : "ok");
  return 0;
}
