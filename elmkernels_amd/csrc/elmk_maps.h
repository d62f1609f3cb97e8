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

// The per-term scan of a CSR map's col (and, with WEIGHTS, w): the first term that fails the column's range, then uniqueness (`unique`:
// no earlier term holds the column), then the weight (finite, with nonneg also >= 0); nnz if none does.  *repeat: it failed uniqueness.
// The loop stops at the first bad term and the caller says why.  Returning texts from inside the loop is slower: the library's build
// switches machine LICM off, so the address of the merged return value is formed again in every iteration.
template <bool WEIGHTS>
inline int64_t csr_scan(int64_t ncols, int64_t nnz, const int32_t* col, const double* w, bool unique, bool nonneg, bool* repeat)
{
  std::vector<char> seen(unique ? (size_t)ncols : 0, 0);
  int64_t p = 0;
  for (; p < nnz; p++) {
    if (col[p] < 0 || col[p] >= ncols) break;
    if (unique && seen[(size_t)col[p]]++) break;
    if (WEIGHTS && (!std::isfinite(w[p]) || (nonneg && !(w[p] >= 0.0)))) break;
  }
  *repeat = p < nnz && col[p] >= 0 && col[p] < ncols && unique && seen[(size_t)col[p]] > 1;
  return p;
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
  bool repeat = false;
  const int64_t p = csr_scan<true>(ncols, nnz, col, w, unique, nonneg, &repeat);
  if (p == nnz) return nullptr;
  if (col[p] < 0 || col[p] >= ncols) return "col outside [0, ncols)";
  if (repeat) return "a column in more than one group (or twice in one)";
  return nonneg ? "weight not finite and >= 0" : "non-finite weight";
}

// Every column in at most one row of a map (elmk_irrigation_supply_enable: the output grid's, which is set without `unique`): the column
// of the first term in CSR order that an earlier term holds already, -1 if there is none, -2 if a column before it is out of range (no
// accepted map).  csr_check's scan with the weights left out.
inline int64_t csr_shared_column(int64_t ncols, int64_t nnz, const int32_t* col)
{
  if (nnz <= 0 || !col) return -1;
  bool repeat = false;
  const int64_t p = csr_scan<false>(ncols, nnz, col, nullptr, true, false, &repeat);
  return p == nnz ? -1 : repeat ? (int64_t)col[p] : -2;
}

// The cell of every column (elmk_floodplain_infiltration_enable; include/elmk.h "floodplain infiltration", F0), from an accepted CSR map by
// cell: cellof[c] = the row whose span names column c, -1 for a column in no row.  Returns csr_shared_column's answer, and fills cellof
// (ncols entries) only where that is -1: a column in two rows has no one cell.
inline int64_t csr_cellof(int64_t nrows, int64_t ncols, const int64_t* ptr, const int32_t* col, std::vector<int32_t>* cellof)
{
  const int64_t nnz = nrows > 0 && ptr ? ptr[nrows] : 0;
  const int64_t shared = csr_shared_column(ncols, nnz, col);
  if (shared != -1) return shared;
  cellof->assign((size_t)(ncols > 0 ? ncols : 0), -1);
  for (int64_t r = 0; r < nrows && nnz > 0 && col; r++)
    for (int64_t p = ptr[r]; p < ptr[r + 1]; p++) (*cellof)[(size_t)col[p]] = (int32_t)r;
  return -1;
}

// River network (elmk_routing_enable; include/elmk.h "runoff routing"): every cell drains into one downstream cell down[c], or is an
// outlet (-1).  ddist: metres to the downstream cell (> 0), area: square metres (>= 0).  Checks, in this order: the arguments; per cell
// in index order the range of down, then a self-loop; the in-degree (at most ROUTE_MAXUP cells drain into one); cycles; ddist; area.
// The cycle check follows every unvisited cell downstream and marks what it passes as on the path (1), then walks the same path again
// and marks it done (2): a path that runs into a cell still marked 1 has closed on itself.  Every cell is marked once each way, so the
// check is linear in ncells, and nothing recurses (a chain as long as the grid is an ordinary network).
// For an accepted network *nup is the largest in-degree (0 .. 8) and up the upstream map as the device reads it: row p of
// ell_npad(*nup) rows of ld >= ncells entries each holds, for cell c, the p-th cell u with down[u] == c in ascending u, else -1.
constexpr int ROUTE_MAXUP = 8;
inline const char* route_check(int64_t ncells, const int32_t* down, const double* ddist, const double* area, int64_t ld, int* nup,
                               std::vector<int32_t>* up)
{
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (!down || !ddist || !area) return "null argument";
  for (int64_t c = 0; c < ncells; c++) {
    if (down[c] < -1 || down[c] >= ncells) return "down outside [-1, ncells)";
    if (down[c] == c) return "down equals its own index";
  }
  std::vector<char> deg((size_t)ncells, 0);
  int most = 0;
  for (int64_t c = 0; c < ncells; c++) {
    if (down[c] < 0) continue;
    char& d = deg[(size_t)down[c]];
    if (d == ROUTE_MAXUP) return "more than 8 upstream cells drain into one cell";
    d++;
    if (d > most) most = d;
  }
  std::vector<char> mark((size_t)ncells, 0);
  for (int64_t c = 0; c < ncells; c++) {
    if (mark[(size_t)c]) continue;
    int64_t j = c;
    for (; j >= 0 && mark[(size_t)j] == 0; j = down[j]) mark[(size_t)j] = 1;
    if (j >= 0 && mark[(size_t)j] == 1) return "the network has a cycle";
    for (j = c; j >= 0 && mark[(size_t)j] == 1; j = down[j]) mark[(size_t)j] = 2;
  }
  for (int64_t c = 0; c < ncells; c++)
    if (!(std::isfinite(ddist[c]) && ddist[c] > 0.0)) return "ddist not finite and > 0";
  for (int64_t c = 0; c < ncells; c++)
    if (!(std::isfinite(area[c]) && area[c] >= 0.0)) return "area not finite and >= 0";
  if (nup) *nup = most;
  if (up) {
    if (ld < ncells) ld = ncells;
    up->assign((size_t)ell_npad(most) * (size_t)ld, -1);
    deg.assign((size_t)ncells, 0);
    for (int64_t u = 0; u < ncells; u++)  // ascending u: each cell's slots fill in ascending order
      if (down[u] >= 0) (*up)[(size_t)deg[(size_t)down[u]]++ * (size_t)ld + (size_t)down[u]] = (int32_t)u;
  }
  return nullptr;
}

// Hillslopes (elmk_hillslope_enable; include/elmk.h "hillslope lateral flow"): every column drains into one downhill column down[c],
// into the stream (-1), or is on no hillslope (-2).  Checks, in this order: the arguments; per column in index order the range of down;
// a self-loop; a column draining into a -2 column; the in-degree (at most ROUTE_MAXUP); cycles, by route_check's linear two-mark walk
// (nothing recurses); then over the hillslope columns (down != -2) in index order, row by row: dist, width, area finite and > 0, elev
// finite; k_aniso finite and > 0.  Returns the text, which names the row, and in *col the first offending column (-1 where the text is
// about no column); the entry point puts " at column <col>" behind the text.  nullptr: accepted.
// For an accepted hillslope set *nup is the largest in-degree (0 .. 8) and up the uphill map as the device reads it: row p of
// ell_npad(*nup) rows of ld >= ncols entries each holds, for column c, the p-th column u with down[u] == c in ascending u, else -1.
inline const char* hillslope_check(int64_t ncols, const int32_t* down, const double* dist, const double* width, const double* area,
                                   const double* elev, double k_aniso, int64_t ld, int* nup, std::vector<int32_t>* up, int64_t* col)
{
  if (col) *col = -1;
  if (ncols < 1 || ncols > INT32_MAX) return "ncols outside 1 .. 2^31-1";
  if (!down || !dist || !width || !area || !elev) return "null argument";
  const auto at = [col](const char* what, int64_t c) {
    if (col) *col = c;
    return what;
  };
  for (int64_t c = 0; c < ncols; c++)
    if (down[c] < -2 || down[c] >= ncols) return at("down outside {-2, -1} and [0, ncols)", c);
  for (int64_t c = 0; c < ncols; c++)
    if (down[c] == c) return at("down equals its own index", c);
  for (int64_t c = 0; c < ncols; c++)
    if (down[c] >= 0 && down[c] != c && down[down[c]] == -2) return at("down names a column on no hillslope", c);
  std::vector<char> deg((size_t)ncols, 0);
  int most = 0;
  for (int64_t c = 0; c < ncols; c++) {
    if (down[c] < 0) continue;
    char& d = deg[(size_t)down[c]];
    if (d == ROUTE_MAXUP) return at("more than 8 uphill columns drain into one column", c);
    d++;
    if (d > most) most = d;
  }
  std::vector<char> mark((size_t)ncols, 0);
  for (int64_t c = 0; c < ncols; c++) {
    if (mark[(size_t)c]) continue;
    int64_t j = c;
    for (; j >= 0 && mark[(size_t)j] == 0; j = down[j]) mark[(size_t)j] = 1;
    if (j >= 0 && mark[(size_t)j] == 1) return at("the hillslope has a cycle", c);
    for (j = c; j >= 0 && mark[(size_t)j] == 1; j = down[j]) mark[(size_t)j] = 2;
  }
  const double* const rows[3] = {dist, width, area};
  static const char* const bad[3] = {"dist not finite and > 0", "width not finite and > 0", "area not finite and > 0"};
  for (int k = 0; k < 3; k++)
    for (int64_t c = 0; c < ncols; c++)
      if (down[c] != -2 && !(std::isfinite(rows[k][c]) && rows[k][c] > 0.0)) return at(bad[k], c);
  for (int64_t c = 0; c < ncols; c++)
    if (down[c] != -2 && !std::isfinite(elev[c])) return at("elev not finite", c);
  if (!(std::isfinite(k_aniso) && k_aniso > 0.0)) return "k_aniso not finite and > 0";
  if (nup) *nup = most;
  if (up) {
    if (ld < ncols) ld = ncols;
    up->assign((size_t)ell_npad(most) * (size_t)ld, -1);
    deg.assign((size_t)ncols, 0);
    for (int64_t u = 0; u < ncols; u++)  // ascending u: each column's slots fill in ascending order
      if (down[u] >= 0) (*up)[(size_t)deg[(size_t)down[u]]++ * (size_t)ld + (size_t)down[u]] = (int32_t)u;
  }
  return nullptr;
}

// Kinematic-wave routing parameters (elmk_routing_kinematic_enable; include/elmk.h "kinematic-wave routing"): params as
// [KINEMATIC_NPARAM][ncells] in the order of ELMK_KW_*, every value finite and > 0.  Checks row by row, in row order; the text names
// the first failing row.  For accepted parameters dev holds the seven rows the device keeps, [7][ld] with ld >= ncells in the order CH,
// CT, CR, TLEN, TWIDTH, RLEN, RWIDTH (elmk_kernels.h: KW_*), padding cells 1.0: CH = (sqrt(HSLP) / NH) * GXR, CT = sqrt(TSLP) / NT,
// CR = sqrt(RSLP) / NR, each operation rounded once.
constexpr int KINEMATIC_NPARAM = 11;
inline const char* kinematic_check(int64_t ncells, const double* params, int64_t ld, std::vector<double>* dev)
{
  static const char* const bad[KINEMATIC_NPARAM] = {
      "HSLP not finite and > 0",   "NH not finite and > 0",   "GXR not finite and > 0",  "TLEN not finite and > 0",
      "TWIDTH not finite and > 0", "TSLP not finite and > 0", "NT not finite and > 0",   "RLEN not finite and > 0",
      "RWIDTH not finite and > 0", "RSLP not finite and > 0", "NR not finite and > 0"};
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (!params) return "null argument";
  const size_t n = (size_t)ncells;
  for (int k = 0; k < KINEMATIC_NPARAM; k++) {
    const double* row = params + (size_t)k * n;
    size_t c = 0;
    for (; c < n; c++)
      if (!(std::isfinite(row[c]) && row[c] > 0.0)) break;
    if (c < n) return bad[k];
  }
  if (dev) {
    if (ld < ncells) ld = ncells;
    const size_t l = (size_t)ld;
    dev->assign((size_t)7 * l, 1.0);
    const double *hslp = params, *nh = params + n, *gxr = params + 2 * n, *tlen = params + 3 * n, *twidth = params + 4 * n,
                 *tslp = params + 5 * n, *nt = params + 6 * n, *rlen = params + 7 * n, *rwidth = params + 8 * n, *rslp = params + 9 * n,
                 *nr = params + 10 * n;
    double* d = dev->data();
    for (size_t c = 0; c < n; c++) {
      d[c] = (std::sqrt(hslp[c]) / nh[c]) * gxr[c];  // (no addition in any of the three: nothing a host compiler could contract)
      d[l + c] = std::sqrt(tslp[c]) / nt[c];
      d[2 * l + c] = std::sqrt(rslp[c]) / nr[c];
      d[3 * l + c] = tlen[c];
      d[4 * l + c] = twidth[c];
      d[5 * l + c] = rlen[c];
      d[6 * l + c] = rwidth[c];
    }
  }
  return nullptr;
}

// Floodplain inundation (elmk_routing_inundation_enable; include/elmk.h "floodplain inundation"): rdepth [ncells], the bank height,
// finite and > 0; eprof [INUNDATION_NPROF][ncells], the elevation profile, finite, eprof[0] == 0.0 and strictly increasing in k.
// Checks, in this order: the arguments; rdepth cell by cell; then per cell in index order the profile: finite (k ascending), its
// first entry, increasing.  Returns the text, which names the row, and in *cell the first offending cell (-1 where the text is about
// no cell); the entry point puts " at cell <cell>" behind the text.  nullptr: accepted.
// For accepted inputs and dev not null, with the cells' area, RLEN and RWIDTH, dev holds I0's tables as the device reads them,
// [25][ld] with ld >= ncells in the order VC, ACHN, AF, E_0 .. E_10, VB_0 .. VB_10 (elmk_kernels.h: FP_*), padding cells 0.0.  VB's
// recurrence has products under sums: compile with -ffp-contract=off, as the library's Makefile does, or the tables may differ from
// the statement's by a rounding.
constexpr int INUNDATION_NPROF = 11;
inline const char* inundation_check(int64_t ncells, const double* rdepth, const double* eprof, const double* area, const double* rlen,
                                    const double* rwidth, int64_t ld, std::vector<double>* dev, int64_t* cell)
{
  if (cell) *cell = -1;
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (!rdepth || !eprof || (dev && (!area || !rlen || !rwidth))) return "null argument";
  const size_t n = (size_t)ncells;
  const auto at = [cell](const char* what, size_t c) {
    if (cell) *cell = (int64_t)c;
    return what;
  };
  for (size_t c = 0; c < n; c++)
    if (!(std::isfinite(rdepth[c]) && rdepth[c] > 0.0)) return at("RDEPTH not finite and > 0", c);
  for (size_t c = 0; c < n; c++) {
    for (int k = 0; k < INUNDATION_NPROF; k++)
      if (!std::isfinite(eprof[(size_t)k * n + c])) return at("EPROF not finite", c);
    if (!(eprof[c] == 0.0)) return at("EPROF[0] not 0", c);
    for (int k = 0; k + 1 < INUNDATION_NPROF; k++)
      if (!(eprof[(size_t)(k + 1) * n + c] > eprof[(size_t)k * n + c])) return at("EPROF not increasing", c);
  }
  if (dev) {
    if (ld < ncells) ld = ncells;
    const size_t l = (size_t)ld;
    dev->assign((size_t)25 * l, 0.0);
    double* d = dev->data();
    for (size_t c = 0; c < n; c++) {  // I0, operation by operation
      const double achn = rlen[c] * rwidth[c];
      const double vc = achn * rdepth[c];
      double af = area[c] - achn;
      if (!(af > 0.0)) af = 0.0;
      d[c] = vc;
      d[l + c] = achn;
      d[2 * l + c] = af;
      double vb = 0.0;
      for (int k = 0; k < INUNDATION_NPROF; k++) {
        const double e = eprof[(size_t)k * n + c];
        d[(size_t)(3 + k) * l + c] = e;
        d[(size_t)(14 + k) * l + c] = vb;
        if (k + 1 < INUNDATION_NPROF) {
          const double fk = (double)k / 10.0, fk1 = (double)(k + 1) / 10.0;
          const double p0 = af * fk, p1 = af * fk1;
          const double s0 = achn + p0, s1 = achn + p1;
          const double de = eprof[(size_t)(k + 1) * n + c] - e;
          const double m = 0.5 * (s0 + s1);
          const double t = m * de;
          vb = vb + t;
        }
      }
    }
  }
  return nullptr;
}

// Reservoirs (elmk_routing_reservoir_enable; include/elmk.h "reservoirs"): cap [ncells], m3, finite and >= 0, 0.0 = no dam;
// target [12][ncells], m3/s, finite and >= 0; beta [ncells] in [0, 1]; mstart [ncells] in 0 .. 11.  Checks, in this order: the
// arguments; cap cell by cell; then per dam cell (cap > 0.0) in index order target (month ascending), beta, mstart.  Returns the
// text, which names the row, and in *cell the first offending cell (-1 where the text is about no cell); the entry point puts
// " at cell <cell>" behind the text.  nullptr: accepted.
// For accepted inputs and dev not null, dev holds the tables as the device reads them, [16][ld] with ld >= ncells in the order CAP,
// SMIN = 0.1 * CAP, C85 = 0.85 * CAP, BETA, TARGET[0 .. 11] (elmk_kernels.h: DAM_*), and mdev MSTART [ld]; padding cells and the
// unchecked rows of cells without a dam 0.
constexpr int RESERVOIR_NMONTH = 12, RESERVOIR_NTAB = 16;
inline const char* reservoir_check(int64_t ncells, const double* cap, const double* target, const double* beta, const int32_t* mstart,
                                   int64_t ld, std::vector<double>* dev, std::vector<int32_t>* mdev, int64_t* cell)
{
  if (cell) *cell = -1;
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (!cap || !target || !beta || !mstart) return "null argument";
  const size_t n = (size_t)ncells;
  const auto at = [cell](const char* what, size_t c) {
    if (cell) *cell = (int64_t)c;
    return what;
  };
  for (size_t c = 0; c < n; c++)
    if (!(std::isfinite(cap[c]) && cap[c] >= 0.0)) return at("CAP not finite and >= 0", c);
  for (size_t c = 0; c < n; c++) {
    if (!(cap[c] > 0.0)) continue;
    for (int m = 0; m < RESERVOIR_NMONTH; m++)
      if (!(std::isfinite(target[(size_t)m * n + c]) && target[(size_t)m * n + c] >= 0.0)) return at("TARGET not finite and >= 0", c);
    if (!(beta[c] >= 0.0 && beta[c] <= 1.0)) return at("BETA outside [0, 1]", c);
    if (mstart[c] < 0 || mstart[c] > 11) return at("MSTART outside 0 .. 11", c);
  }
  if (dev && mdev) {
    if (ld < ncells) ld = ncells;
    const size_t l = (size_t)ld;
    dev->assign((size_t)RESERVOIR_NTAB * l, 0.0);
    mdev->assign(l, 0);
    double* d = dev->data();
    for (size_t c = 0; c < n; c++) {
      if (!(cap[c] > 0.0)) continue;
      d[c] = cap[c];
      d[l + c] = 0.1 * cap[c];
      d[2 * l + c] = 0.85 * cap[c];
      d[3 * l + c] = beta[c];
      for (int m = 0; m < RESERVOIR_NMONTH; m++) d[(size_t)(4 + m) * l + c] = target[(size_t)m * n + c];
      (*mdev)[c] = mstart[c];
    }
  }
  return nullptr;
}

// Stream temperature (elmk_routing_heat_enable; include/elmk.h "stream temperature"): sublev in 0 .. 14; shade [ncells] in [0, 1], or
// null for 0.0 everywhere.  Checks, in this order: ncells, sublev, shade cell by cell.  Returns the text, which names the row, and in
// *cell the first offending cell (-1 where the text is about no cell); the entry point puts " at cell <cell>" behind the text.
// nullptr: accepted.  For accepted inputs and dev not null, dev holds H0's KSW = (1.0 - ALBW) * (1.0 - SHADE) as the device reads it,
// [ld] with ld >= ncells; padding cells 0.
constexpr int HEAT_NSUBLEV = 15;
constexpr double HEAT_ALBW = 0.1;
inline const char* heat_check(int64_t ncells, int sublev, const double* shade, int64_t ld, std::vector<double>* dev, int64_t* cell)
{
  if (cell) *cell = -1;
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (sublev < 0 || sublev >= HEAT_NSUBLEV) return "sublev outside 0 .. 14";
  const size_t n = (size_t)ncells;
  if (shade)
    for (size_t c = 0; c < n; c++)
      if (!(shade[c] >= 0.0 && shade[c] <= 1.0)) {
        if (cell) *cell = (int64_t)c;
        return "SHADE outside [0, 1]";
      }
  if (dev) {
    if (ld < ncells) ld = ncells;
    dev->assign((size_t)ld, 0.0);
    for (size_t c = 0; c < n; c++) (*dev)[c] = (1.0 - HEAT_ALBW) * (1.0 - (shade ? shade[c] : 0.0));
  }
  return nullptr;
}

// Command areas (elmk_routing_command_enable; include/elmk.h "command areas"): cap [ncells], the reservoirs' CAP (a dam: > 0.0), and
// the cells' three ELL rows [COMMAND_NDEP][ncells]: dam, int32, the cell of a supplying dam or -1 for an empty slot, filled from slot 0
// without gaps; share in (0, 1]; claim in [0, 1].  Checks, in this order: the arguments; per cell in index order and per slot in slot
// order: the index in range, no filled slot behind an empty one, a cell with a reservoir, not the cell itself, not a dam of an earlier
// slot, share, claim; behind the slots the cell's shares added in slot order; then per dam in the order of the dam list its claims
// added in the order of its terms.  Returns the text, which names the row, and in *cell the first offending cell - for the claims' sum
// the dam's cell - (-1 where the text is about no cell); the entry point puts " at cell <cell>" behind the text.  nullptr: accepted.
// For accepted inputs and out not null, out holds what the device reads: the ELL rows [COMMAND_NDEP][ld] with ld >= ncells (padding
// cells and empty slots: dam -1, share and claim 0.0) and the inverse map - dams: every cell with cap > 0.0 in ascending order, those
// without dependents included; ptr [ndams + 1]; the terms (cell, slot) sorted by cell and then slot, with their share.  Linear time, no
// recursion: one count per dam, a prefix sum, and one pass over the cells in index order.
constexpr int COMMAND_NDEP = 4;
struct CommandTables {
  std::vector<int32_t> dam;          // [COMMAND_NDEP][ld]
  std::vector<double> share, claim;  // [COMMAND_NDEP][ld]
  std::vector<int32_t> dams;         // [ndams]
  std::vector<int64_t> ptr;          // [ndams + 1]
  std::vector<int32_t> tcell, tslot;  // [nterms]
  std::vector<double> tshare;         // [nterms]
};
inline const char* command_check(int64_t ncells, const double* cap, const int32_t* dam, const double* share, const double* claim, int64_t ld,
                                 CommandTables* out, int64_t* cell)
{
  if (cell) *cell = -1;
  if (ncells < 1 || ncells > INT32_MAX) return "ncells outside 1 .. 2^31-1";
  if (!cap || !dam || !share || !claim) return "null argument";
  const size_t n = (size_t)ncells;
  const auto at = [cell](const char* what, size_t c) {
    if (cell) *cell = (int64_t)c;
    return what;
  };
  std::vector<int64_t> count(n, 0);  // per cell: the terms of the dam that stands there
  for (size_t c = 0; c < n; c++) {
    bool empty = false;
    double sum = 0.0;
    for (int k = 0; k < COMMAND_NDEP; k++) {
      const int64_t d = dam[(size_t)k * n + c];
      if (d < -1 || d >= ncells) return at("DAM outside [-1, ncells)", c);
      if (d < 0) {
        empty = true;
        continue;
      }
      if (empty) return at("DAM filled behind an empty slot", c);
      if (!(cap[d] > 0.0)) return at("DAM names a cell without a reservoir", c);
      if (d == (int64_t)c) return at("DAM names the cell itself", c);
      for (int j = 0; j < k; j++)
        if (dam[(size_t)j * n + c] == d) return at("DAM names one reservoir twice", c);
      const double s = share[(size_t)k * n + c], q = claim[(size_t)k * n + c];
      if (!(std::isfinite(s) && s > 0.0 && s <= 1.0)) return at("SHARE outside (0, 1]", c);
      if (!(q >= 0.0 && q <= 1.0)) return at("CLAIM outside [0, 1]", c);
      sum = k == 0 ? s : sum + s;
      count[(size_t)d]++;
    }
    if (!(sum <= 1.0)) return at("SHARE sums to more than 1", c);
  }
  CommandTables T;
  std::vector<int64_t> slot_of(n, -1);  // per cell: its place in the dam list
  for (size_t c = 0; c < n; c++)
    if (cap[c] > 0.0) {
      slot_of[c] = (int64_t)T.dams.size();
      T.dams.push_back((int32_t)c);
    }
  T.ptr.assign(T.dams.size() + 1, 0);
  for (size_t j = 0; j < T.dams.size(); j++) T.ptr[j + 1] = T.ptr[j] + count[(size_t)T.dams[j]];
  const size_t nnz = (size_t)T.ptr.back();
  T.tcell.assign(nnz, 0);
  T.tslot.assign(nnz, 0);
  T.tshare.assign(nnz, 0.0);
  std::vector<double> tclaim(nnz, 0.0);
  std::vector<int64_t> fill(T.ptr.begin(), T.ptr.end() - 1);
  for (size_t c = 0; c < n; c++)  // cells ascending, slots ascending: every dam's terms come out sorted by cell and then slot
    for (int k = 0; k < COMMAND_NDEP; k++) {
      const int64_t d = dam[(size_t)k * n + c];
      if (d < 0) break;
      const size_t p = (size_t)fill[(size_t)slot_of[(size_t)d]]++;
      T.tcell[p] = (int32_t)c;
      T.tslot[p] = k;
      T.tshare[p] = share[(size_t)k * n + c];
      tclaim[p] = claim[(size_t)k * n + c];
    }
  for (size_t j = 0; j < T.dams.size(); j++) {
    double sum = 0.0;
    for (int64_t p = T.ptr[j]; p < T.ptr[j + 1]; p++) sum = p == T.ptr[j] ? tclaim[(size_t)p] : sum + tclaim[(size_t)p];
    if (!(sum <= 1.0)) return at("CLAIM sums to more than 1", (size_t)T.dams[j]);
  }
  if (out) {
    if (ld < ncells) ld = ncells;
    const size_t l = (size_t)ld;
    T.dam.assign((size_t)COMMAND_NDEP * l, -1);
    T.share.assign((size_t)COMMAND_NDEP * l, 0.0);
    T.claim.assign((size_t)COMMAND_NDEP * l, 0.0);
    for (size_t c = 0; c < n; c++)
      for (int k = 0; k < COMMAND_NDEP; k++) {
        const int32_t d = dam[(size_t)k * n + c];
        if (d < 0) break;
        T.dam[(size_t)k * l + c] = d;
        T.share[(size_t)k * l + c] = share[(size_t)k * n + c];
        T.claim[(size_t)k * l + c] = claim[(size_t)k * n + c];
      }
    *out = std::move(T);
  }
  return nullptr;
}

// The reservoirs' calendar, the reference's no-leap year: the month 0 .. 11 of day-of-year doy (0 = 1 January; any other doy is taken
// modulo 365), and whether a step with (doy, decday) starts at 00:00 of the first day of its month: the active layer's rollover test,
// decday == doy + 1.0, on the first doy of each month.
inline int reservoir_month(int64_t doy)
{
  static const int first[13] = {0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334, 365};
  const int d = (int)(((doy % 365) + 365) % 365);
  int m = 0;
  while (d >= first[m + 1]) m++;
  return m;
}
inline bool reservoir_month_begins(int64_t doy, double decday)
{
  static const int first[12] = {0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334};
  if (doy < 0 || doy > 364 || !(decday == (double)doy + 1.0)) return false;
  return first[reservoir_month(doy)] == (int)doy;
}

}  // namespace elmk
