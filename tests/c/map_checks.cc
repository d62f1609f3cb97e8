// The host checks of the two map shapes (elmkernels_amd/csrc/elmk_maps.h), case by case: prints "<case>: <returned text>", or
// "<case>: ok" for an accepted map.  tests/test_map_checks_host.py compares every line with the message the entry points give.
#include "elmk_maps.h"

#include <cstdio>
#include <limits>
#include <vector>

using namespace elmk;

namespace {
const double NaN = std::numeric_limits<double>::quiet_NaN();
const double Inf = std::numeric_limits<double>::infinity();

void say(const char* name, const char* text) { printf("%s: %s\n", name, text ? text : "ok"); }

// an ELL map of 3 columns over 4 cells: row 0 valid, the other rows padding; then one entry changed
constexpr int64_t NCOLS = 3, NCELLS = 4;
struct Ell {
  int npts;
  std::vector<int32_t> idx;
  std::vector<double> w;
  explicit Ell(int n) : npts(n), idx((size_t)n * NCOLS, -1), w((size_t)n * NCOLS, 0.0)
  {
    for (int c = 0; c < NCOLS; c++) {
      idx[c] = c + 1;
      w[c] = 1.0;
    }
  }
  Ell& set(int k, int c, int32_t i, double wt = 0.5)
  {
    idx[(size_t)k * NCOLS + c] = i;
    w[(size_t)k * NCOLS + c] = wt;
    return *this;
  }
  const char* check(int64_t ncells = NCELLS) const { return ell_check(NCOLS, ncells, npts, idx.data(), w.data()); }
};

// a CSR map of 3 rows over 3 columns
constexpr int64_t NROWS = 3;
// the two callers' rules: output cells (repeats allowed, finite weights) and groups (a column once, weights >= 0)
#define CELLS "ncells outside 1 .. 2^31-1", false, false
#define GROUPS "ngroups outside 1 .. 2^31-1", true, true
const char* csr(const std::vector<int64_t>& ptr, const std::vector<int32_t>& col, const std::vector<double>& w, const char* bad_nrows, bool unique,
                bool nonneg)
{
  return csr_check(NROWS, NCOLS, ptr.data(), col.empty() ? nullptr : col.data(), w.empty() ? nullptr : w.data(), bad_nrows, unique, nonneg);
}
}  // namespace

int main()
{
  for (int n = 1; n <= 8; n++) printf("ell_npad(%d): %d\n", n, ell_npad(n));

  const Ell one(1);
  say("ell npts 0", ell_check(NCOLS, NCELLS, 0, one.idx.data(), one.w.data()));
  say("ell npts 9", ell_check(NCOLS, NCELLS, 9, one.idx.data(), one.w.data()));
  say("ell ncells 0", one.check(0));
  say("ell ncells 2^31", one.check((int64_t)1 << 31));
  say("ell null idx", ell_check(NCOLS, NCELLS, 1, nullptr, one.w.data()));
  say("ell null w", ell_check(NCOLS, NCELLS, 1, one.idx.data(), nullptr));
  say("ell idx[0] -1", Ell(2).set(0, 1, -1).check());
  say("ell idx[0] ncells", Ell(2).set(0, 2, (int32_t)NCELLS).check());
  say("ell idx[1] -2", Ell(2).set(1, 0, -2).check());
  say("ell idx[1] ncells", Ell(2).set(1, 2, (int32_t)NCELLS).check());
  say("ell NaN weight", Ell(2).set(1, 1, 0, NaN).check());
  say("ell inf weight", Ell(1).set(0, 2, 3, Inf).check());
  say("ell NaN behind padding", Ell(2).set(1, 1, -1, NaN).check());
  say("ell no columns", ell_check(0, NCELLS, 2, nullptr, nullptr));
  say("ell valid 1", Ell(1).check());
  say("ell valid 2", Ell(2).set(1, 0, 0).check());
  say("ell valid 3", Ell(3).set(1, 0, 0).set(2, 0, 3).set(2, 2, 0).check());
  Ell eight(8);
  for (int k = 1; k < 8; k++)
    for (int c = 0; c < NCOLS; c++) eight.set(k, c, (k + c) % (int32_t)NCELLS, 0.125);
  say("ell valid 8", eight.check());
  // two checks violated at once: the first in (row, column) order wins, and the argument checks come before the map's
  say("ell bad weight in row 0, bad idx in row 1", Ell(2).set(0, 2, 0, NaN).set(1, 0, -2).check());
  say("ell bad idx and bad weight in one row", Ell(2).set(1, 0, 1, Inf).set(1, 1, -2).check());
  say("ell npts 0 and ncells 0", ell_check(NCOLS, 0, 0, nullptr, nullptr));

  const std::vector<int64_t> ptr{0, 1, 2, 3};
  const std::vector<int32_t> col{2, 0, 1};
  const std::vector<double> w{1.0, 0.5, 0.25};
  say("csr nrows 0, cells", csr_check(0, NCOLS, ptr.data(), col.data(), w.data(), CELLS));
  say("csr nrows 0, groups", csr_check(0, NCOLS, ptr.data(), col.data(), w.data(), GROUPS));
  say("csr null ptr", csr_check(NROWS, NCOLS, nullptr, col.data(), w.data(), CELLS));
  say("csr ptr[0] 1", csr({1, 1, 2, 3}, col, w, CELLS));
  say("csr ptr decreasing", csr({0, 2, 1, 3}, col, w, CELLS));
  say("csr nnz 2^31", csr({0, (int64_t)1 << 31, (int64_t)1 << 31, (int64_t)1 << 31}, {}, {}, CELLS));
  say("csr null col", csr_check(NROWS, NCOLS, ptr.data(), nullptr, w.data(), CELLS));
  say("csr null w", csr_check(NROWS, NCOLS, ptr.data(), col.data(), nullptr, GROUPS));
  say("csr col -1", csr(ptr, {2, -1, 1}, w, CELLS));
  say("csr col ncols", csr(ptr, {2, 0, (int32_t)NCOLS}, w, GROUPS));
  say("csr repeated column, unique", csr(ptr, {2, 0, 2}, w, GROUPS));
  say("csr repeated column, repeats allowed", csr(ptr, {2, 0, 2}, w, CELLS));
  say("csr NaN weight, cells", csr(ptr, col, {1.0, NaN, 0.25}, CELLS));
  say("csr NaN weight, groups", csr(ptr, col, {1.0, NaN, 0.25}, GROUPS));
  say("csr weight -1, non-negative", csr(ptr, col, {1.0, -1.0, 0.25}, GROUPS));
  say("csr weight -1, finite only", csr(ptr, col, {1.0, -1.0, 0.25}, CELLS));
  say("csr empty rows", csr({0, 0, 3, 3}, col, w, GROUPS));
  say("csr nnz 0", csr({0, 0, 0, 0}, {}, {}, GROUPS));
  // per term: the column's range, then uniqueness, then the weight
  say("csr repeated column with a bad weight", csr(ptr, {2, 0, 2}, {1.0, 0.5, NaN}, GROUPS));
  say("csr bad column with a bad weight", csr(ptr, {2, 0, 7}, {1.0, 0.5, NaN}, GROUPS));
  return 0;
}
