// api_routing.cpp - runoff routing (k_routing.hip; include/elmk.h "runoff routing"): the cell rows VOLR, QIN, QOUT, QOUT_SUM over the
// output grid's cells, the network's parameter rows and upstream map and the budget's reduction scratch, in one allocation held
// exactly while the feature is enabled; and the stage's second scheme, kinematic-wave routing (include/elmk.h "kinematic-wave
// routing"), whose rows WH, WT, QSUR and derived parameters live in a second allocation held exactly while that scheme is on; and that
// scheme's floodplain inundation (include/elmk.h "floodplain inundation"), whose rows WF, FLOOD_DEPTH, FLOOD_FRAC and tables live in a
// third, held exactly while the extension is on; and its reservoirs (include/elmk.h "reservoirs"), whose rows RES, KRLS, RES_TAKE and
// tables live in a fourth, held exactly while that extension is on.
#include "elmk_ctx.h"

namespace {
// ELMK_ROUTE_* -> the row of the allocation (the budget's three rows lie first: elmk_kernels.h)
constexpr int ROUTE_ROW_OF[4] = {ROUTE_VOLR, ROUTE_QIN, ROUTE_QOUT, ROUTE_QOUT_SUM};
static_assert(ELMK_ROUTE_VOLR == 0 && ELMK_ROUTE_QIN == 1 && ELMK_ROUTE_QOUT == 2 && ELMK_ROUTE_QOUT_SUM == 3, "four rows");
// the kinematic-wave scheme's public rows are the first three of its own allocation
static_assert(ELMK_ROUTE_WH - 4 == KW_WH && ELMK_ROUTE_WT - 4 == KW_WT && ELMK_ROUTE_QSUR - 4 == KW_QSUR, "three rows");
static_assert(ELMK_KW_NPARAM == KINEMATIC_NPARAM, "the parameter rows of elmk_maps.h");
// the floodplain inundation's public rows are the rows of its own allocation
static_assert(ELMK_ROUTE_WF - 7 == FP_WF && ELMK_ROUTE_FLOOD_DEPTH - 7 == FP_DEPTH && ELMK_ROUTE_FLOOD_FRAC - 7 == FP_FRAC, "three rows");
static_assert(ELMK_FP_NPROF == INUNDATION_NPROF && FP_VB - FP_E == ELMK_FP_NPROF && FP_NTAB - FP_VB == ELMK_FP_NPROF, "the profile of elmk_maps.h");

// the reservoirs' public rows -> the rows of their own allocation (the budget's two rows lie first: elmk_kernels.h)
constexpr int DAM_ROW_OF[3] = {DAM_RES, DAM_KRLS, DAM_TAKE};
static_assert(ELMK_ROUTE_RES == 10 && ELMK_ROUTE_KRLS == 11 && ELMK_ROUTE_RES_TAKE == 12, "three rows");
static_assert(DAM_NTAB == RESERVOIR_NTAB && DAM_TARGET + RESERVOIR_NMONTH == DAM_NTAB, "the tables of elmk_maps.h");

RouteArgs route_args(const elmk_ctx* ctx)
{
  const elmk_ctx::Routing& T = ctx->route;
  return RouteArgs{T.ncells, T.cld, T.npad, T.nsub, T.rows, T.kout, T.area, T.up};
}

int route_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  return ctx->route.mem ? ELMK_OK : invalid(ctx, (std::string(who) + ": not enabled (elmk_routing_enable)").c_str());
}

int kinematic_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = route_enter(ctx, who)) return rc;
  return ctx->route.kw_mem ? ELMK_OK : invalid(ctx, (std::string(who) + ": the scheme is not on (elmk_routing_kinematic_enable)").c_str());
}

int inundation_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = kinematic_enter(ctx, who)) return rc;
  return ctx->route.fp_mem ? ELMK_OK : invalid(ctx, (std::string(who) + ": the extension is not on (elmk_routing_inundation_enable)").c_str());
}

int reservoir_enter(elmk_ctx* ctx, const char* who)
{
  if (int rc = kinematic_enter(ctx, who)) return rc;
  return ctx->route.dam_mem ? ELMK_OK : invalid(ctx, (std::string(who) + ": the extension is not on (elmk_routing_reservoir_enable)").c_str());
}

void reservoir_off(elmk_ctx::Routing& T)
{
  T.dam_mem = DevBuf<char>{};
  T.dam_rows = T.dam_tab = nullptr;
  T.dam_mstart = nullptr;
  T.dam_time = 0;
}

void inundation_off(elmk_ctx::Routing& T)
{
  T.fp_mem = DevBuf<char>{};
  T.fp_rows = T.fp_tab = nullptr;
}
}  // namespace

namespace elmk {
void route_launch(elmk_ctx* ctx, double dt, bool run)
{
  const elmk_ctx::Routing& T = ctx->route;
  const CsrMap& M = ctx->ogrid.map;
  const size_t ld = (size_t)ctx->ld;
  const OGridMap G{M.ptr, M.col, M.w, M.nrows, 0.0};
  const double* const qrunoff = ctx->wb_rows + (size_t)ELMK_WB_QRUNOFF * ld;
  const double* const qirr = T.withdraw ? ctx->irr_rows + (size_t)ELMK_IRR_QFLX_IRRIG * ld : nullptr;
  if (T.kw_mem)  // the scheme switch: the kinematic-wave scheme exactly while its memory is held
    launch_routing_kinematic(route_args(ctx), KinematicArgs{T.kw_rows, T.kw_par}, FloodArgs{T.fp_rows, T.fp_tab},
                             DamArgs{T.dam_rows, T.dam_tab, T.dam_mstart, run ? ctx->run.table : nullptr, run ? ctx->run.cursor : nullptr,
                                     T.dam_time},
                             G, qrunoff, qirr, ctx->hyd_rows + (size_t)ELMK_HYD_QFLX_SURF * ld, ctx->hyd_rows + (size_t)ELMK_HYD_QFLX_H2OSFC_SURF * ld, dt,
                             ctx->stream);
  else
    launch_routing(route_args(ctx), G, qrunoff, qirr, dt, ctx->stream);
}

const double* route_row(const elmk_ctx* ctx, int which, const char** why)
{
  const elmk_ctx::Routing& T = ctx->route;
  if (!T.mem) return *why = "runoff routing is not enabled (elmk_routing_enable)", nullptr;
  if (which < 0 || which > ELMK_ROUTE_RES_TAKE) return *why = "row out of range", nullptr;
  if (which >= ELMK_ROUTE_RES)  // (the reservoirs' rows are in range exactly while they are on)
    return T.dam_mem ? T.dam_rows + (size_t)DAM_ROW_OF[which - ELMK_ROUTE_RES] * (size_t)T.cld : (*why = "row out of range", nullptr);
  if (which > ELMK_ROUTE_QSUR && !T.fp_mem) return *why = "the floodplain inundation is not on (elmk_routing_inundation_enable)", nullptr;
  if (which > ELMK_ROUTE_QOUT_SUM && !T.kw_mem) return *why = "the kinematic-wave scheme is not on (elmk_routing_kinematic_enable)", nullptr;
  return which > ELMK_ROUTE_QSUR       ? T.fp_rows + (size_t)(which - ELMK_ROUTE_WF) * (size_t)T.cld
         : which > ELMK_ROUTE_QOUT_SUM ? T.kw_rows + (size_t)(which - ELMK_ROUTE_WH) * (size_t)T.cld
                                       : T.rows + (size_t)ROUTE_ROW_OF[which] * (size_t)T.cld;
}

int route_holds(elmk_ctx* ctx, const char* who, bool with_withdrawal)
{
  if (!ctx->route.mem || (with_withdrawal && !ctx->route.withdraw)) return ELMK_OK;
  return invalid(ctx, (std::string(who) + ": runoff routing is enabled" + (with_withdrawal ? " with the withdrawal on" : "") +
                       " (elmk_routing_clear first)").c_str());
}
}  // namespace elmk

extern "C" {

int elmk_routing_enable(elmk_ctx* ctx, int64_t ncells, const int32_t* down, const double* ddist, const double* area, double effvel, int nsub)
{
  const char* who = "elmk_routing_enable";
  if (int rc = enter(ctx)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (!ctx->ogrid.mem) return invalid(ctx, "elmk_routing_enable: no output grid (elmk_set_output_grid)");
  if (ncells != ctx->ogrid.map.nrows) return invalid(ctx, "elmk_routing_enable: ncells differs from the output grid's");
  if (!ctx->wb_rows) return invalid(ctx, "elmk_routing_enable: the water balance is not enabled (elmk_water_balance_enable)");
  if (T.mem) return invalid(ctx, "elmk_routing_enable: already enabled");
  if (!(std::isfinite(effvel) && effvel > 0.0)) return invalid(ctx, "elmk_routing_enable: effvel not finite and > 0");
  if (nsub < 1 || nsub > 64) return invalid(ctx, "elmk_routing_enable: nsub outside 1 .. 64");
  const int64_t cld = (ncells + 63) / 64 * 64;
  int nup = 0;
  std::vector<int32_t> up;
  // (every gather of k_routing_step stays inside a cell row because of this check)
  if (int rc = invalid_map(ctx, who, route_check(ncells, down, ddist, area, cld, &nup, &up))) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the stages of its flags' moment)
  const int npad = ell_npad(nup);
  T = elmk_ctx::Routing{};
  if (hip_fail(ctx, carve(T.mem, [&](Carve& L) {
                 L.take(T.rows, (size_t)ROUTE_NROWS * cld * sizeof(double));
                 L.take(T.kout, (size_t)cld * sizeof(double));
                 L.take(T.area, (size_t)cld * sizeof(double));
                 L.take(T.up, (size_t)npad * cld * sizeof(int32_t));
                 L.take(T.down, (size_t)cld * sizeof(int32_t));
                 L.take(T.part, (size_t)3 * ELMK_CONS_NPART * 3 * sizeof(double));
                 L.take(T.out, 256);
               }), "hipMalloc(runoff routing)")) {
    T = elmk_ctx::Routing{};
    return ELMK_E_NOMEM;
  }
  std::vector<double> kout((size_t)ncells);
  for (int64_t c = 0; c < ncells; c++) kout[(size_t)c] = effvel / ddist[c];
  const size_t n = (size_t)ncells;
  // everything zero, the padding cells of down -1, then the network
  if (hip_fail(ctx, hipMemsetAsync(T.mem, 0, T.mem.bytes(), ctx->stream), "hipMemset(runoff routing)") ||
      hip_fail(ctx, hipMemsetAsync(T.down, 0xFF, (size_t)cld * sizeof(int32_t), ctx->stream), "hipMemset(runoff routing down)") ||
      hip_fail(ctx, hipMemcpyAsync(T.kout, kout.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(runoff routing KOUT)") ||
      hip_fail(ctx, hipMemcpyAsync(T.area, area, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(runoff routing area)") ||
      hip_fail(ctx, hipMemcpyAsync(T.up, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(runoff routing up)") ||
      hip_fail(ctx, hipMemcpyAsync(T.down, down, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(runoff routing down)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    T = elmk_ctx::Routing{};
    return ELMK_E_HIP;
  }
  T.ncells = ncells;
  T.cld = cld;
  T.npad = npad;
  T.nsub = nsub;
  return ELMK_OK;
}

int elmk_routing_init(elmk_ctx* ctx, const double* volr, const double* qout_sum, int64_t ncalls)
{
  const char* who = "elmk_routing_init";
  if (int rc = route_enter(ctx, who)) return rc;
  if (ncalls < 0) return invalid(ctx, "elmk_routing_init: ncalls is negative");
  if (int rc = refuse_capture(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  HIPCHK(hipMemsetAsync(T.rows, 0, (size_t)ROUTE_NROWS * cld * sizeof(double), ctx->stream));
  if (volr) HIPCHK(hipMemcpyAsync(T.rows + ROUTE_VOLR * cld, volr, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (qout_sum) HIPCHK(hipMemcpyAsync(T.rows + ROUTE_QOUT_SUM * cld, qout_sum, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = synced(ctx)) return rc;
  T.ncalls = ncalls;
  return ELMK_OK;
}

int elmk_routing(elmk_ctx* ctx, double dt)
{
  if (int rc = route_enter(ctx, "elmk_routing")) return rc;
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_routing: dt must be finite and positive");
  route_launch(ctx, dt);
  ctx->route.ncalls++;
  return launched(ctx);
}

int elmk_routing_read(elmk_ctx* ctx, int which, double* host, int64_t cell0, int64_t n)
{
  const char* who = "elmk_routing_read";
  if (int rc = route_enter(ctx, who)) return rc;
  const elmk_ctx::Routing& T = ctx->route;
  const bool dam_row = which >= ELMK_ROUTE_RES && which <= ELMK_ROUTE_RES_TAKE;
  if (dam_row ? !T.dam_mem : which < 0 || which > (T.fp_mem ? ELMK_ROUTE_FLOOD_FRAC : T.kw_mem ? ELMK_ROUTE_QSUR : ELMK_ROUTE_QOUT_SUM))
    return invalid(ctx, "elmk_routing_read: unknown row");
  if (int rc = check_range(ctx, who, host, cell0, n, T.ncells, "cell")) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  const double* const row = dam_row                       ? T.dam_rows + (size_t)DAM_ROW_OF[which - ELMK_ROUTE_RES] * (size_t)T.cld
                            : which > ELMK_ROUTE_QSUR     ? T.fp_rows + (size_t)(which - ELMK_ROUTE_WF) * (size_t)T.cld
                            : which > ELMK_ROUTE_QOUT_SUM ? T.kw_rows + (size_t)(which - ELMK_ROUTE_WH) * (size_t)T.cld
                                                          : T.rows + (size_t)ROUTE_ROW_OF[which] * (size_t)T.cld;
  if (n > 0) HIPCHK(hipMemcpyAsync(host, row + (size_t)cell0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int elmk_routing_count(elmk_ctx* ctx, int64_t* ncalls)
{
  if (int rc = route_enter(ctx, "elmk_routing_count")) return rc;
  if (!ncalls) return invalid(ctx, "elmk_routing_count: null argument");
  *ncalls = ctx->route.ncalls;
  return ELMK_OK;
}

int elmk_routing_reset_mean(elmk_ctx* ctx)
{
  if (int rc = route_enter(ctx, "elmk_routing_reset_mean")) return rc;
  elmk_ctx::Routing& T = ctx->route;
  HIPCHK(hipMemsetAsync(T.rows + ROUTE_QOUT_SUM * (size_t)T.cld, 0, (size_t)T.cld * sizeof(double), ctx->stream));
  T.ncalls = 0;
  return ELMK_OK;
}

int elmk_routing_set_withdrawal(elmk_ctx* ctx, int on)
{
  const char* who = "elmk_routing_set_withdrawal";
  if (int rc = route_enter(ctx, who)) return rc;
  if (on && !ctx->irr_rows) return invalid(ctx, "elmk_routing_set_withdrawal: the irrigation is not enabled (elmk_irrigation_enable)");
  if (!on)
    if (int rc = irrsup_holds(ctx, who)) return rc;  // (the limit grants water that only the withdrawal takes out of VOLR)
  if (int rc = refuse_capture(ctx, who)) return rc;
  ctx->route.withdraw = on != 0;  // (the captured run step is keyed by it)
  return ELMK_OK;
}

int elmk_routing_budget(elmk_ctx* ctx, double* sums)
{
  const char* who = "elmk_routing_budget";
  if (int rc = route_enter(ctx, who)) return rc;
  if (!sums) return invalid(ctx, "elmk_routing_budget: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const elmk_ctx::Routing& T = ctx->route;
  launch_routing_outlets(route_args(ctx), T.down, ctx->stream);
  launch_min_max_sum(T.rows, T.cld, T.ncells, 3, T.part, T.out, ctx->stream);
  HIPCHK(hipGetLastError());
  double mms[9];
  HIPCHK(hipMemcpyAsync(mms, T.out, sizeof mms, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 3; k++) sums[k] = mms[3 * k + 2];
  return ELMK_OK;
}

int elmk_routing_kinematic_enable(elmk_ctx* ctx, const double* params)
{
  const char* who = "elmk_routing_kinematic_enable";
  if (int rc = route_enter(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_routing_kinematic_enable: the soil hydrology is not enabled (elmk_soil_hydrology_enable)");
  if (T.kw_mem) return invalid(ctx, "elmk_routing_kinematic_enable: already on");
  std::vector<double> par;
  if (int rc = invalid_map(ctx, who, kinematic_check(T.ncells, params, T.cld, &par))) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the scheme of its moment)
  const size_t cld = (size_t)T.cld;
  const auto off = [&] {
    T.kw_mem = DevBuf<char>{};
    T.kw_rows = T.kw_par = nullptr;
  };
  if (hip_fail(ctx, carve(T.kw_mem, [&](Carve& L) {
                 L.take(T.kw_rows, (size_t)KW_NROWS * cld * sizeof(double));
                 L.take(T.kw_par, (size_t)KW_NPAR * cld * sizeof(double));
               }), "hipMalloc(kinematic-wave routing)")) {
    off();
    return ELMK_E_NOMEM;
  }
  if (hip_fail(ctx, hipMemsetAsync(T.kw_mem, 0, T.kw_mem.bytes(), ctx->stream), "hipMemset(kinematic-wave routing)") ||
      hip_fail(ctx, hipMemcpyAsync(T.kw_par, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream),
               "hipMemcpy(kinematic-wave routing parameters)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    off();
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

int elmk_routing_kinematic_init(elmk_ctx* ctx, const double* wh, const double* wt)
{
  const char* who = "elmk_routing_kinematic_init";
  if (int rc = kinematic_enter(ctx, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  HIPCHK(hipMemsetAsync(T.kw_rows, 0, (size_t)KW_NROWS * cld * sizeof(double), ctx->stream));
  if (wh) HIPCHK(hipMemcpyAsync(T.kw_rows + KW_WH * cld, wh, n * 8, hipMemcpyHostToDevice, ctx->stream));
  if (wt) HIPCHK(hipMemcpyAsync(T.kw_rows + KW_WT * cld, wt, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_routing_kinematic_budget(elmk_ctx* ctx, double* sums)
{
  const char* who = "elmk_routing_kinematic_budget";
  if (int rc = kinematic_enter(ctx, who)) return rc;
  if (!sums) return invalid(ctx, "elmk_routing_kinematic_budget: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const elmk_ctx::Routing& T = ctx->route;
  launch_min_max_sum(T.kw_rows, T.cld, T.ncells, 2, T.part, T.out, ctx->stream);  // K8 (the routing's partials: both budgets synchronise)
  HIPCHK(hipGetLastError());
  double mms[6];
  HIPCHK(hipMemcpyAsync(mms, T.out, sizeof mms, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 2; k++) sums[k] = mms[3 * k + 2];
  return ELMK_OK;
}

int elmk_routing_kinematic_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_routing_kinematic_clear")) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (!T.kw_mem) return ELMK_OK;
  if (T.fp_mem)  // (the extension's tables are formed from the scheme's RLEN and RWIDTH, and its kernel is the scheme's)
    return invalid(ctx, "elmk_routing_kinematic_clear: the floodplain inundation is on (elmk_routing_inundation_clear first)");
  if (T.dam_mem)  // (the reservoirs' kernel is the scheme's)
    return invalid(ctx, "elmk_routing_kinematic_clear: the reservoirs are on (elmk_routing_reservoir_clear first)");
  if (int rc = cellrows_hold(ctx, "elmk_routing_kinematic_clear", ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_WH, ELMK_ROUTE_QSUR)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  T.kw_mem = DevBuf<char>{};
  T.kw_rows = T.kw_par = nullptr;
  return ELMK_OK;
}

int elmk_routing_inundation_enable(elmk_ctx* ctx, const double* rdepth, const double* eprof)
{
  const char* who = "elmk_routing_inundation_enable";
  if (int rc = kinematic_enter(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (T.fp_mem) return invalid(ctx, "elmk_routing_inundation_enable: already on");
  if (!rdepth || !eprof) return invalid(ctx, "elmk_routing_inundation_enable: null argument");
  {
    int64_t cell = -1;
    const char* const text = inundation_check(T.ncells, rdepth, eprof, nullptr, nullptr, nullptr, T.cld, nullptr, &cell);
    if (text && cell >= 0) return invalid_map(ctx, who, (std::string(text) + " at cell " + std::to_string(cell)).c_str());
    if (int rc = invalid_map(ctx, who, text)) return rc;
  }
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the form of its moment)
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  // I0 reads the cells' area and the scheme's RLEN and RWIDTH: the device holds the only copies
  std::vector<double> area(n), rlen(n), rwidth(n), tab;
  if (hip_fail(ctx, hipMemcpyAsync(area.data(), T.area, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(area)") ||
      hip_fail(ctx, hipMemcpyAsync(rlen.data(), T.kw_par + KW_RLEN * cld, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(RLEN)") ||
      hip_fail(ctx, hipMemcpyAsync(rwidth.data(), T.kw_par + KW_RWIDTH * cld, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(RWIDTH)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    return ELMK_E_HIP;
  }
  (void)inundation_check(T.ncells, rdepth, eprof, area.data(), rlen.data(), rwidth.data(), T.cld, &tab, nullptr);
  if (hip_fail(ctx, carve(T.fp_mem, [&](Carve& L) {
                 L.take(T.fp_rows, (size_t)FP_NROWS * cld * sizeof(double));
                 L.take(T.fp_tab, (size_t)FP_NTAB * cld * sizeof(double));
               }), "hipMalloc(floodplain inundation)")) {
    inundation_off(T);
    return ELMK_E_NOMEM;
  }
  if (hip_fail(ctx, hipMemsetAsync(T.fp_mem, 0, T.fp_mem.bytes(), ctx->stream), "hipMemset(floodplain inundation)") ||
      hip_fail(ctx, hipMemcpyAsync(T.fp_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream),
               "hipMemcpy(floodplain inundation tables)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    inundation_off(T);
    return ELMK_E_HIP;
  }
  return ELMK_OK;
}

int elmk_routing_inundation_init(elmk_ctx* ctx, const double* wf)
{
  const char* who = "elmk_routing_inundation_init";
  if (int rc = inundation_enter(ctx, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  HIPCHK(hipMemsetAsync(T.fp_rows, 0, (size_t)FP_NROWS * cld * sizeof(double), ctx->stream));
  if (wf) HIPCHK(hipMemcpyAsync(T.fp_rows + FP_WF * cld, wf, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);
}

int elmk_routing_inundation_budget(elmk_ctx* ctx, double* sums)
{
  const char* who = "elmk_routing_inundation_budget";
  if (int rc = inundation_enter(ctx, who)) return rc;
  if (!sums) return invalid(ctx, "elmk_routing_inundation_budget: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const elmk_ctx::Routing& T = ctx->route;
  launch_min_max_sum(T.fp_rows, T.cld, T.ncells, 1, T.part, T.out, ctx->stream);  // I7 (the routing's partials: every budget synchronises)
  HIPCHK(hipGetLastError());
  double mms[3];
  HIPCHK(hipMemcpyAsync(mms, T.out, sizeof mms, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  sums[0] = mms[2];
  return ELMK_OK;
}

int elmk_routing_inundation_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_routing_inundation_clear")) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (!T.fp_mem) return ELMK_OK;
  if (int rc = cellrows_hold(ctx, "elmk_routing_inundation_clear", ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_WF, ELMK_ROUTE_FLOOD_FRAC)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  inundation_off(T);
  return ELMK_OK;
}

int elmk_routing_reservoir_enable(elmk_ctx* ctx, const double* cap, const double* target, const double* beta, const int32_t* mstart)
{
  const char* who = "elmk_routing_reservoir_enable";
  if (int rc = kinematic_enter(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (T.dam_mem) return invalid(ctx, "elmk_routing_reservoir_enable: already on");
  if (!cap || !target || !beta || !mstart) return invalid(ctx, "elmk_routing_reservoir_enable: null argument");
  std::vector<double> tab;
  std::vector<int32_t> ms;
  {
    int64_t cell = -1;
    const char* const text = reservoir_check(T.ncells, cap, target, beta, mstart, T.cld, &tab, &ms, &cell);
    if (text && cell >= 0) return invalid_map(ctx, who, (std::string(text) + " at cell " + std::to_string(cell)).c_str());
    if (int rc = invalid_map(ctx, who, text)) return rc;
  }
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the form of its moment)
  const size_t cld = (size_t)T.cld;
  if (hip_fail(ctx, carve(T.dam_mem, [&](Carve& L) {
                 L.take(T.dam_rows, (size_t)DAM_NROWS * cld * sizeof(double));
                 L.take(T.dam_tab, (size_t)DAM_NTAB * cld * sizeof(double));
                 L.take(T.dam_mstart, cld * sizeof(int32_t));
               }), "hipMalloc(reservoirs)")) {
    reservoir_off(T);
    return ELMK_E_NOMEM;
  }
  std::vector<double> one(cld, 1.0);  // KRLS starts at 1.0, as _init leaves it
  if (hip_fail(ctx, hipMemsetAsync(T.dam_mem, 0, T.dam_mem.bytes(), ctx->stream), "hipMemset(reservoirs)") ||
      hip_fail(ctx, hipMemcpyAsync(T.dam_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream),
               "hipMemcpy(reservoir tables)") ||
      hip_fail(ctx, hipMemcpyAsync(T.dam_mstart, ms.data(), ms.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream),
               "hipMemcpy(reservoir MSTART)") ||
      hip_fail(ctx, hipMemcpyAsync(T.dam_rows + DAM_KRLS * cld, one.data(), cld * sizeof(double), hipMemcpyHostToDevice, ctx->stream),
               "hipMemcpy(reservoir KRLS)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    reservoir_off(T);
    return ELMK_E_HIP;
  }
  T.dam_time = 0;
  return ELMK_OK;
}

int elmk_routing_reservoir_init(elmk_ctx* ctx, const double* res, const double* krls)
{
  const char* who = "elmk_routing_reservoir_init";
  if (int rc = reservoir_enter(ctx, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  elmk_ctx::Routing& T = ctx->route;
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  std::vector<double> one(cld, 1.0);
  HIPCHK(hipMemsetAsync(T.dam_rows, 0, (size_t)DAM_NROWS * cld * sizeof(double), ctx->stream));
  HIPCHK(hipMemcpyAsync(T.dam_rows + DAM_KRLS * cld, krls ? krls : one.data(), (krls ? n : cld) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (res) HIPCHK(hipMemcpyAsync(T.dam_rows + DAM_RES * cld, res, n * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);  // (`one` lives until here)
}

int elmk_routing_reservoir_time(elmk_ctx* ctx, int month, int begins)
{
  const char* who = "elmk_routing_reservoir_time";
  if (int rc = reservoir_enter(ctx, who)) return rc;
  if (month < 0 || month > 11) return invalid(ctx, "elmk_routing_reservoir_time: month outside 0 .. 11");
  if (int rc = refuse_capture(ctx, who)) return rc;
  ctx->route.dam_time = (int32_t)(month | (begins ? 16 : 0));  // (a kernel argument of the stepwise call; the run's step reads its pad word)
  return ELMK_OK;
}

int elmk_routing_reservoir_budget(elmk_ctx* ctx, double* sums)
{
  const char* who = "elmk_routing_reservoir_budget";
  if (int rc = reservoir_enter(ctx, who)) return rc;
  if (!sums) return invalid(ctx, "elmk_routing_reservoir_budget: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const elmk_ctx::Routing& T = ctx->route;
  launch_min_max_sum(T.dam_rows, T.cld, T.ncells, 2, T.part, T.out, ctx->stream);  // D6 (the routing's partials: every budget synchronises)
  HIPCHK(hipGetLastError());
  double mms[6];
  HIPCHK(hipMemcpyAsync(mms, T.out, sizeof mms, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 2; k++) sums[k] = mms[3 * k + 2];
  return ELMK_OK;
}

int elmk_routing_reservoir_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_routing_reservoir_clear")) return rc;
  elmk_ctx::Routing& T = ctx->route;
  if (!T.dam_mem) return ELMK_OK;
  if (int rc = cellrows_hold(ctx, "elmk_routing_reservoir_clear", ELMK_CELL_ROWS_ROUTING, ELMK_ROUTE_RES, ELMK_ROUTE_RES_TAKE)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  reservoir_off(T);
  return ELMK_OK;
}

int elmk_routing_clear(elmk_ctx* ctx)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, "elmk_routing_clear")) return rc;
  if (!ctx->route.mem) return ELMK_OK;
  if (int rc = irrsup_holds(ctx, "elmk_routing_clear")) return rc;  // (the limit reads VOLR and area)
  if (int rc = cellrows_hold(ctx, "elmk_routing_clear")) return rc;  // (every cell row lies in an allocation this call frees)
  if (int rc = quiesce(ctx, false)) return rc;
  ctx->route = elmk_ctx::Routing{};
  return ELMK_OK;
}

}  // extern "C"
