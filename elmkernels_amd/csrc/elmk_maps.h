// elmk_maps.h - the two map shapes the host API takes from a caller, each checked in one place.  Host code only: no HIP, no context,
// so a host compiler builds it alone (tests/c/map_checks.cc).
// These checks are all that keeps the gathers of the remap, deposition, aggregate and renormalisation kernels inside their
// buffers.  Each returns the text of the first failing check, which the entry point puts behind its own name ("elmk_xxx: "), or
// nullptr for a map the kernels may read.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

namespace elmk {

// ELL map, per column: idx (int32) and w (fp64) as [npts][ncols]; idx -1 is padding, never in row 0.  On the device the rows are
// padded to npad = 1, 2, 4 or 8 (the widths the kernels are instantiated for).
inline int ell_npad(int npts) { return npts <= 1 ? 1 : npts <= 2 ? 2 : npts <= 4 ? 4 : 8; }

inline const char* ell_check(int64_t ncols, int64_t ncells, int npts, const int32_t* idx, const double* w)
{
  if (npts < 1 || npts > 8) return "npts outside 1 .. 8";
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (ncols > 0 && (!idx || !w)) return "null map";
  for (int k = 0; k < npts; k++) {  // row by row: both arrays are read in memory order
    const int32_t* ik = idx + (size_t)k * ncols;
    const double* wk = w + (size_t)k * ncols;
    const int32_t lo = k == 0 ? 0 : -1;
    for (int64_t c = 0; c < ncols; c++) {
      if (ik[c] < lo || ik[c] >= ncells) return k == 0 ? "idx[0] outside [0, ncells)" : "idx outside [-1, ncells)";
      if (ik[c] >= 0 && !std::isfinite(wk[c])) return "non-finite weight";
    }
  }
  return nullptr;
}

// CSR map, by row (an output cell, a group): ptr (int64, nrows + 1), col (int32, nnz = ptr[nrows]: columns), w (fp64, nnz).
// bad_nrows: the message for nrows outside 1 .. 2^31-1 (it names the caller's rows); unique: a column appears at most once in the
// whole map; nonneg: weights are >= 0 as well as finite.  Per term the column's range, then uniqueness, then the weight.
inline const char* csr_check(int64_t nrows, int64_t ncols, const int64_t* ptr, const int32_t* col, const double* w, const char* bad_nrows,
                             bool unique, bool nonneg)
{
  if (nrows < 1 || nrows > INT32_MAX) return bad_nrows;
  if (!ptr) return "null ptr";
  if (ptr[0] != 0) return "ptr[0] != 0";
  for (int64_t i = 0; i < nrows; i++)
    if (ptr[i + 1] < ptr[i]) return "ptr decreasing";
  const int64_t nnz = ptr[nrows];
  if (nnz > INT32_MAX) return "nnz outside 0 .. 2^31-1";
  if (nnz > 0 && (!col || !w)) return "null map";
  // The loop stops at the first bad term and the lines after it say why.  Returning the texts from inside the loop is slower: the
  // library's build switches machine LICM off, so the address of the merged return value is formed again in every iteration.
  std::vector<char> seen(unique ? (size_t)ncols : 0, 0);
  int64_t p = 0;
  for (; p < nnz; p++) {
    if (col[p] < 0 || col[p] >= ncols) break;
    if (unique && seen[(size_t)col[p]]++) break;
    if (!std::isfinite(w[p]) || (nonneg && !(w[p] >= 0.0))) break;
  }
  if (p == nnz) return nullptr;
  if (col[p] < 0 || col[p] >= ncols) return "col outside [0, ncols)";
  if (unique && seen[(size_t)col[p]] > 1) return "a column in more than one group (or twice in one)";
  return nonneg ? "weight not finite and >= 0" : "non-finite weight";
}

}  // namespace elmk
