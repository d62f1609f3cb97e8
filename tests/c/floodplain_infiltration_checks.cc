// The host check of elmk_floodplain_infiltration_enable (elmkernels_amd/csrc/elmk_maps.h: csr_cellof; include/elmk.h "floodplain
// infiltration", F0), case by case: prints "<case>: <returned value>[ <cellof ...>]" - -1 and the cell of every column (-1 for a column
// in no cell) for a map with every column in at most one cell, else the first column an earlier term holds already (-2: a column out of
// range before any repeat) and no cells, since a shared column has no one cell.  tests/test_floodplain_infiltration_host.py compares
// every line with tests/floodplain_infiltration_cases.py: cellof.
#include "elmk_maps.h"

#include <cstdio>
#include <vector>

using namespace elmk;

namespace {
void say(const char* name, int64_t ncols, const std::vector<int64_t>& ptr, const std::vector<int32_t>& col, bool show = true)
{
  std::vector<int32_t> cellof{7, 7, 7};  // (what it held goes, or stays untouched under a refusal)
  const int64_t rc = csr_cellof((int64_t)ptr.size() - 1, ncols, ptr.data(), col.empty() ? nullptr : col.data(), &cellof);
  printf("%s: %lld", name, (long long)rc);
  if (rc == -1) {
    if (show)
      for (int32_t g : cellof) printf(" %d", g);
    else {
      long long sum = 0, none = 0;
      for (int32_t g : cellof) sum += g, none += g < 0;
      printf(" size=%zu sum=%lld none=%lld", cellof.size(), sum, none);
    }
  } else if (cellof.size() != 3 || cellof[0] != 7) {
    printf(" (cellof written)");
  }
  printf("\n");
}
}  // namespace

int main()
{
  say("one column in one cell", 1, {0, 1}, {0});
  say("one cell without terms", 3, {0, 0}, {});
  say("every column once", 5, {0, 2, 2, 5}, {3, 0, 4, 1, 2});
  say("columns in no cell", 9, {0, 1, 2}, {8, 0});
  say("empty cells around a full one", 4, {0, 0, 0, 3, 3}, {2, 0, 3});
  say("last column twice", 5, {0, 2, 4}, {0, 4, 1, 4});
  say("twice in one cell", 5, {0, 3}, {0, 0, 1});
  say("two repeats, the first in term order wins", 6, {0, 3, 6}, {5, 2, 3, 2, 5, 3});
  say("column out of range before a repeat", 4, {0, 3}, {0, 4, 0});
  say("column negative before a repeat", 4, {0, 1, 3}, {0, -1, 0});
  say("repeat before a column out of range", 4, {0, 3}, {0, 0, 9});
  say("no columns at all", 0, {0, 0}, {});
  // a long map: 100 000 columns once each in reverse order over 1000 cells of 100, then column 77 again as one more term of the last
  std::vector<int32_t> big(100000);
  std::vector<int64_t> ptr(1001);
  for (size_t i = 0; i < big.size(); i++) big[i] = (int32_t)(big.size() - 1 - i);
  for (size_t r = 0; r < ptr.size(); r++) ptr[r] = (int64_t)r * 100;
  say("100000 columns over 1000 cells", 100000, ptr, big, false);
  say("... under 100003 columns", 100003, ptr, big, false);
  big.push_back(77);
  ptr.back() += 1;
  say("... and one again", 100000, ptr, big, false);
  return 0;
}
