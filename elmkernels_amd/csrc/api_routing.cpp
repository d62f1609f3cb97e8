// api_routing.cpp - the river stage (k_routing.hip; include/elmk.h "runoff routing", "kinematic-wave routing", "floodplain inundation",
// "reservoirs", "stream temperature", "floodplain infiltration", "command areas").  The stage has seven parts, each with one allocation held exactly while the part is on (elmk_ctx.h: Routing): the
// base part, the kinematic-wave scheme on top of it, and that scheme's three extensions.  The table PARTS describes each part once - its
// rows, its public row ids, what its budget reduces, what the restart image keeps of it, what it needs and how its refusals read - and
// the part_* helpers below are what the five families of entry points share: how a call enters, how an enable, an init, a budget and a
// clear go.  An entry point keeps what is its own: its argument checks and the arrays it uploads.
#include "elmk_ctx.h"

namespace {
using Routing = elmk_ctx::Routing;

enum { BASE, KW, FP, DAM, HEAT, LAND, CMD, NPARTS };
struct PartDesc {
  Routing::Part Routing::*at;  // where the part is held (null: the base part, in Routing itself)
  int needs;                   // the part that has to be on before this one (-1: none)
  int nrows;                   // the rows of its allocation
  int id0, nids, row_of[7];    // its public rows ELMK_ROUTE_* id0 .. id0 + nids - 1, and the row of the allocation behind each
  int nbudget;                 // its budget reduces this many leading rows (elmk_kernels.h lays them first)
  int nstate, state[2];        // its prognostic rows (ELMK_ROUTE_*) in the order of the restart image
  const char* label;           // in the text of a HIP error
  const char *enable, *clear;  // its calls, as the refusals name them
  const char* off;             // "<who>: <off> (<enable>)": a call that needs the part while it is off
  const char* row_off;         // route_row's text for one of its rows while it is off
  const char* on;              // "<who>: <on> (<clear> first)": a call that needs it off
};
constexpr PartDesc PARTS[NPARTS] = {
    {nullptr, -1, ROUTE_NROWS, ELMK_ROUTE_VOLR, 4, {ROUTE_VOLR, ROUTE_QIN, ROUTE_QOUT, ROUTE_QOUT_SUM}, 3, 2, {ELMK_ROUTE_VOLR, ELMK_ROUTE_QOUT_SUM},
     "runoff routing", "elmk_routing_enable", "elmk_routing_clear", "not enabled", "runoff routing is not enabled (elmk_routing_enable)",
     "runoff routing is enabled"},
    {&Routing::kw, BASE, KW_NROWS, ELMK_ROUTE_WH, 3, {KW_WH, KW_WT, KW_QSUR}, 2, 2, {ELMK_ROUTE_WH, ELMK_ROUTE_WT},
     "kinematic-wave routing", "elmk_routing_kinematic_enable", "elmk_routing_kinematic_clear", "the scheme is not on",
     "the kinematic-wave scheme is not on (elmk_routing_kinematic_enable)", nullptr},  // (elmk_routing_clear takes the scheme with it)
    // (the extension's tables are formed from the scheme's RLEN and RWIDTH, and its kernel is the scheme's)
    {&Routing::fp, KW, FP_NROWS, ELMK_ROUTE_WF, 3, {FP_WF, FP_DEPTH, FP_FRAC}, 1, 1, {ELMK_ROUTE_WF},
     "floodplain inundation", "elmk_routing_inundation_enable", "elmk_routing_inundation_clear", "the extension is not on",
     "the floodplain inundation is not on (elmk_routing_inundation_enable)", "the floodplain inundation is on"},
    // (the reservoirs' kernel is the scheme's; their rows are in range exactly while they are on)
    {&Routing::dam, KW, DAM_NROWS, ELMK_ROUTE_RES, 3, {DAM_RES, DAM_KRLS, DAM_TAKE}, 2, 2, {ELMK_ROUTE_RES, ELMK_ROUTE_KRLS},
     "reservoirs", "elmk_routing_reservoir_enable", "elmk_routing_reservoir_clear", "the extension is not on", "row out of range",
     "the reservoirs are on"},
    // (the stream temperature's kernel is the scheme's; it excludes the two extensions before it: heat_excludes)
    {&Routing::heat, KW, HT_NROWS, ELMK_ROUTE_TT, 7, {HT_TT, HT_TR, HT_HEAT, HT_HIN, HT_HSRF, HT_HADJ, HT_HOUT}, 5, 2, {ELMK_ROUTE_TT, ELMK_ROUTE_TR},
     "stream temperature", "elmk_routing_heat_enable", "elmk_routing_heat_clear", "the extension is not on", "row out of range",
     "the stream temperature is on"},
    // (the floodplain infiltration: its cell row QLAND; the three column rows and cellof lie behind it in the same allocation)
    // (F1 reads FLOOD_FRAC as the last call left it, so with the extension on the image keeps that row as well: state)
    {&Routing::land, FP, 1, ELMK_ROUTE_QLAND, 1, {0}, 1, 1, {ELMK_ROUTE_FLOOD_FRAC}, "floodplain infiltration", "elmk_floodplain_infiltration_enable",
     "elmk_floodplain_infiltration_clear", "the extension is not on", "row out of range", "the floodplain infiltration is on"},
    // (the command areas: four diagnostic rows, nothing in the image; C5 reduces GIVE and TAKE, which lie first)
    {&Routing::cmd, DAM, CMD_NROWS, ELMK_ROUTE_CMD_WANT, 4, {CMD_WANT, CMD_TAKE, CMD_GIVE, CMD_RATIO}, 2, 0, {0}, "command areas",
     "elmk_routing_command_enable", "elmk_routing_command_clear", "the command areas are not on", "row out of range", "the command areas are on"}};
static_assert(ELMK_ROUTE_VOLR == 0 && ELMK_ROUTE_QIN == 1 && ELMK_ROUTE_QOUT == 2 && ELMK_ROUTE_QOUT_SUM == 3, "four rows");
static_assert(ELMK_ROUTE_WH - 4 == KW_WH && ELMK_ROUTE_WT - 4 == KW_WT && ELMK_ROUTE_QSUR - 4 == KW_QSUR, "three rows");
static_assert(ELMK_KW_NPARAM == KINEMATIC_NPARAM, "the parameter rows of elmk_maps.h");
static_assert(ELMK_ROUTE_WF - 7 == FP_WF && ELMK_ROUTE_FLOOD_DEPTH - 7 == FP_DEPTH && ELMK_ROUTE_FLOOD_FRAC - 7 == FP_FRAC, "three rows");
static_assert(ELMK_FP_NPROF == INUNDATION_NPROF && FP_VB - FP_E == ELMK_FP_NPROF && FP_NTAB - FP_VB == ELMK_FP_NPROF, "the profile of elmk_maps.h");
static_assert(ELMK_ROUTE_RES == 10 && ELMK_ROUTE_KRLS == 11 && ELMK_ROUTE_RES_TAKE == 12, "three rows");
static_assert(DAM_NTAB == RESERVOIR_NTAB && DAM_TARGET + RESERVOIR_NMONTH == DAM_NTAB, "the tables of elmk_maps.h");
static_assert(ELMK_ROUTE_TT == 13 && ELMK_ROUTE_HOUT == 19 && HT_HEAT == 0 && HT_HIN == 1 && HT_HSRF == 2 && HT_HADJ == 3 && HT_OUTLET == 4, "seven rows; H7's five lead");
static_assert(HEAT_NSUBLEV == 15, "the soil layers of elmk_maps.h");
static_assert(ELMK_ROUTE_CMD_WANT == 21 && ELMK_ROUTE_CMD_RATIO == 24 && ELMK_CMD_NDEP == COMMAND_NDEP && CMD_NDEP == COMMAND_NDEP, "four rows, four slots");
static_assert(PARTS[CMD].nstate == 0, "the command areas keep nothing in the image");
// (the heat excludes the inundation and the reservoirs, so the image never holds more than the rows of the first four parts and the last)
static_assert(PARTS[0].nstate + PARTS[1].nstate + PARTS[2].nstate + PARTS[3].nstate + PARTS[5].nstate == elmk::ROUTE_STATE_MAX &&
                  PARTS[0].nstate + PARTS[1].nstate + PARTS[4].nstate <= elmk::ROUTE_STATE_MAX, "the rows of the image");

const DevBuf<char>& part_mem(const Routing& T, const PartDesc& P) { return P.at ? (T.*P.at).mem : T.mem; }
double* part_rows(const Routing& T, const PartDesc& P) { return P.at ? (T.*P.at).rows : T.rows; }

RouteArgs route_args(const elmk_ctx* ctx)
{
  const Routing& T = ctx->route;
  return RouteArgs{T.ncells, T.cld, T.npad, T.nsub, T.rows, T.kout, T.area, T.up};
}

// how every call that needs part p begins: the refusal of the part it needs comes before its own
int part_enter(elmk_ctx* ctx, int p, const char* who)
{
  const PartDesc& P = PARTS[p];
  if (int rc = P.needs < 0 ? enter(ctx) : part_enter(ctx, P.needs, who)) return rc;
  return part_mem(ctx->route, P) ? ELMK_OK : invalid(ctx, (std::string(who) + ": " + P.off + " (" + P.enable + ")").c_str());
}

void part_reset(Routing& T, int p)
{
  if (p == BASE) T = Routing{};  // (and every other part with it)
  else T.*PARTS[p].at = Routing::Part{};
  if (p == DAM) T.dam_mstart = nullptr, T.dam_time = 0;
  if (p == HEAT) T.heat_sublev = 0;
  if (p == LAND) T.land_cellof = nullptr;
  if (p == CMD) {
    T.cmd_ones = T.cmd_tshare = nullptr;
    T.cmd_dam = T.cmd_dams = T.cmd_tcell = nullptr;
    T.cmd_ptr = nullptr;
    T.cmd_ndams = 0;
  }
}

// the heat and the scheme's two other extensions exclude each other: "<who>: <on> (<clear> first)" while part q is on
int part_excludes(elmk_ctx* ctx, int q, const char* who)
{
  const PartDesc& Q = PARTS[q];
  return part_mem(ctx->route, Q) ? invalid(ctx, (std::string(who) + ": " + Q.on + " (" + Q.clear + " first)").c_str()) : ELMK_OK;
}

// one host array onto the device, enqueued; true: it failed (what: in the error's text)
template <class V>
bool upload(elmk_ctx* ctx, V* dev, const V* host, size_t n, const char* what)
{
  return hip_fail(ctx, hipMemcpyAsync(dev, host, n * sizeof(V), hipMemcpyHostToDevice, ctx->stream), what);
}

// how an enable ends: the part's allocation laid out and zeroed, then the caller's uploads (true: one failed), then a wait.  A failure
// leaves the part off.
template <class Layout, class Uploads>
int part_on(elmk_ctx* ctx, int p, Layout layout, Uploads uploads)
{
  Routing& T = ctx->route;
  const PartDesc& P = PARTS[p];
  DevBuf<char>& mem = P.at ? (T.*P.at).mem : T.mem;
  const std::string label = std::string("(") + P.label + ")";
  int rc = ELMK_OK;
  if (hip_fail(ctx, carve(mem, layout), ("hipMalloc" + label).c_str())) {
    rc = ELMK_E_NOMEM;
  } else if (hip_fail(ctx, hipMemsetAsync(mem, 0, mem.bytes(), ctx->stream), ("hipMemset" + label).c_str()) || uploads() ||
             hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    rc = ELMK_E_HIP;
  }
  if (rc) part_reset(T, p);
  return rc;
}

// a refusal of elmk_maps.h's checks that names a cell: "<who>: <text> at cell N"
int invalid_at(elmk_ctx* ctx, const char* who, const char* text, int64_t cell)
{
  return text && cell >= 0 ? invalid_map(ctx, who, (std::string(text) + " at cell " + std::to_string(cell)).c_str()) : invalid_map(ctx, who, text);
}

int part_zero(elmk_ctx* ctx, int p)
{
  const Routing& T = ctx->route;
  HIPCHK(hipMemsetAsync(part_rows(T, PARTS[p]), 0, (size_t)PARTS[p].nrows * (size_t)T.cld * sizeof(double), ctx->stream));
  if (p == CMD)  // (RATIO's rest state is 1.0)
    HIPCHK(hipMemcpyAsync(T.cmd.rows + (size_t)CMD_RATIO * (size_t)T.cld, T.cmd_ones, (size_t)T.cld * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return ELMK_OK;
}

// how an init goes on after its checks: every row of the part zero, then the caller's rows (a null one stays zero); enqueued
struct HostRow {
  int row;
  const double* host;
};
int part_init(elmk_ctx* ctx, int p, std::initializer_list<HostRow> rows)
{
  const Routing& T = ctx->route;
  if (int rc = part_zero(ctx, p)) return rc;
  for (const HostRow& r : rows)
    if (r.host)
      HIPCHK(hipMemcpyAsync(part_rows(T, PARTS[p]) + (size_t)r.row * (size_t)T.cld, r.host, (size_t)T.ncells * 8, hipMemcpyHostToDevice, ctx->stream));
  return ELMK_OK;
}

// a part's budget (R6, K8, I7, D6): the sums of its leading rows, through the base part's partials - every budget synchronises
int part_budget(elmk_ctx* ctx, int p, const char* who, double* sums)
{
  if (int rc = part_enter(ctx, p, who)) return rc;
  if (!sums) return invalid(ctx, (std::string(who) + ": null argument").c_str());
  if (int rc = refuse_capture(ctx, who)) return rc;
  const Routing& T = ctx->route;
  const int n = PARTS[p].nbudget;
  if (p == BASE) launch_routing_outlets(route_args(ctx), T.down, ctx->stream);  // (R6's third row)
  if (p == HEAT)  // (H7's fifth row)
    launch_routing_outlet_row(T.down, T.heat.rows + (size_t)HT_HOUT * (size_t)T.cld, T.heat.rows + (size_t)HT_OUTLET * (size_t)T.cld, T.ncells, ctx->stream);
  double mms[18];
  // (the base part's partials hold three rows: a longer budget goes through them three rows at a time, in stream order)
  for (int k0 = 0; k0 < n; k0 += 3) {
    const int m = n - k0 < 3 ? n - k0 : 3;
    launch_min_max_sum(part_rows(T, PARTS[p]) + (size_t)k0 * (size_t)T.cld, T.cld, T.ncells, m, T.part, T.out, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(mms + 3 * k0, T.out, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIPCHK(hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; k++) sums[k] = mms[3 * k + 2];
  return ELMK_OK;
}

// a part's clear: nothing to do while it is off; refused while something needs it; then the part's reset under an idle stream
int part_clear(elmk_ctx* ctx, int p, const char* who)
{
  if (int rc = enter(ctx)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  Routing& T = ctx->route;
  const PartDesc& P = PARTS[p];
  if (!part_mem(T, P)) return ELMK_OK;
  if (p == BASE) {  // (the other parts go with it; the supply limit reads VOLR and area)
    if (int rc = irrsup_holds(ctx, who)) return rc;
  } else {
    for (const PartDesc& Q : PARTS)
      if (Q.needs == p && part_mem(T, Q)) return invalid(ctx, (std::string(who) + ": " + Q.on + " (" + Q.clear + " first)").c_str());
  }
  // (base: every cell row lies in an allocation this call frees)
  if (int rc = p == BASE ? cellrows_hold(ctx, who) : cellrows_hold(ctx, who, ELMK_CELL_ROWS_ROUTING, P.id0, P.id0 + P.nids - 1)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;
  part_reset(T, p);
  return ELMK_OK;
}
}  // namespace

namespace elmk {
void route_launch(elmk_ctx* ctx, double dt, bool run)
{
  const Routing& T = ctx->route;
  const CsrMap& M = ctx->ogrid.map;
  const size_t ld = (size_t)ctx->ld;
  const OGridMap G{M.ptr, M.col, M.w, M.nrows, 0.0};
  const double* const qrunoff = ctx->wb_rows + (size_t)ELMK_WB_QRUNOFF * ld;
  const double* const qirr = T.withdraw ? ctx->irr_rows + (size_t)ELMK_IRR_QFLX_IRRIG * ld : nullptr;
  if (T.kw.mem) {  // the scheme switch: the kinematic-wave scheme exactly while its memory is held
    HeatArgs H{};
    if (T.heat.mem) {
      H.rows = T.heat.rows;
      H.ksw = T.heat.tab;
      static const int fields[HTF_N] = {ELMK_FIELD_forc_tbot, ELMK_FIELD_forc_pbot, ELMK_FIELD_forc_qbot,  ELMK_FIELD_forc_lwrad, ELMK_FIELD_forc_u,
                                        ELMK_FIELD_forc_v,    ELMK_FIELD_forc_solad, ELMK_FIELD_forc_solai, ELMK_FIELD_t_grnd,     ELMK_FIELD_t_soisno};
      for (int k = 0; k < HTF_N; k++) H.fields[k] = ctx->fptr[fields[k]];
      H.dtype = store_dtype(ELMK_F64);
      H.sublev = T.heat_sublev;
      H.ld = ctx->ld;
    }
    launch_routing_kinematic(route_args(ctx), KinematicArgs{T.kw.rows, T.kw.tab}, FloodArgs{T.fp.rows, T.fp.tab},
                             DamArgs{T.dam.rows, T.dam.tab, T.dam_mstart, run ? ctx->run.table : nullptr, run ? ctx->run.cursor : nullptr,
                                     T.dam_time},
                             H, G, qrunoff, qirr, ctx->hyd_rows + (size_t)ELMK_HYD_QFLX_SURF * ld, ctx->hyd_rows + (size_t)ELMK_HYD_QFLX_H2OSFC_SURF * ld, dt,
                             ctx->stream, LandArgs{T.land.mem ? T.land.tab + (size_t)ELMK_FPI_QFLX_DRAIN * ld : nullptr, T.land.rows},
                             T.cmd.mem ? CmdArgs{T.cmd.rows, T.cmd_dam, T.cmd.tab, T.cmd.tab + (size_t)CMD_NDEP * (size_t)T.cld, T.cmd_dams, T.cmd_ptr,
                                                 T.cmd_tcell, T.cmd_tshare, T.cmd_ndams}
                                       : CmdArgs{});
  } else {
    launch_routing(route_args(ctx), G, qrunoff, qirr, dt, ctx->stream);
  }
}

const double* route_row(const elmk_ctx* ctx, int which, const char** why)
{
  const Routing& T = ctx->route;
  if (!T.mem) return *why = PARTS[BASE].row_off, nullptr;
  for (const PartDesc& P : PARTS)
    if (which >= P.id0 && which < P.id0 + P.nids)
      return part_mem(T, P) ? part_rows(T, P) + (size_t)P.row_of[which - P.id0] * (size_t)T.cld : (*why = P.row_off, nullptr);
  return *why = "row out of range", nullptr;
}

int land_holds(elmk_ctx* ctx, const char* who)
{
  return ctx->route.land.mem ? part_excludes(ctx, LAND, who) : ELMK_OK;
}

int route_holds(elmk_ctx* ctx, const char* who, bool with_withdrawal)
{
  if (!ctx->route.mem || (with_withdrawal && !ctx->route.withdraw)) return ELMK_OK;
  return invalid(ctx, (std::string(who) + ": " + PARTS[BASE].on + (with_withdrawal ? " with the withdrawal on" : "") + " (" + PARTS[BASE].clear +
                       " first)").c_str());
}

size_t route_bytes(const elmk_ctx* ctx)
{
  size_t bytes = 0;
  for (const PartDesc& P : PARTS) bytes += part_mem(ctx->route, P).bytes();
  return bytes;
}

int route_zero_rows(elmk_ctx* ctx)
{
  for (int p = 0; p < NPARTS; p++)
    if (part_mem(ctx->route, PARTS[p]))
      if (int rc = part_zero(ctx, p)) return rc;
  return ELMK_OK;
}

int route_state_rows(const elmk_ctx* ctx, int* ids)
{
  if (!ctx->restart_cells || !ctx->route.mem) return 0;
  int n = 0;
  for (const PartDesc& P : PARTS)
    if (part_mem(ctx->route, P))
      for (int k = 0; k < P.nstate; k++) ids[n++] = P.state[k];
  return n;
}
}  // namespace elmk

extern "C" {

int elmk_routing_enable(elmk_ctx* ctx, int64_t ncells, const int32_t* down, const double* ddist, const double* area, double effvel, int nsub)
{
  const char* who = "elmk_routing_enable";
  if (int rc = enter(ctx)) return rc;
  Routing& T = ctx->route;
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
  const size_t n = (size_t)ncells;
  std::vector<double> kout(n);
  for (size_t c = 0; c < n; c++) kout[c] = effvel / ddist[c];
  T = Routing{};
  T.ncells = ncells;
  T.cld = cld;
  T.npad = npad;
  T.nsub = nsub;
  return part_on(
      ctx, BASE,
      [&](Carve& L) {
        L.take(T.rows, (size_t)ROUTE_NROWS * cld * sizeof(double));
        L.take(T.kout, (size_t)cld * sizeof(double));
        L.take(T.area, (size_t)cld * sizeof(double));
        L.take(T.up, (size_t)npad * cld * sizeof(int32_t));
        L.take(T.down, (size_t)cld * sizeof(int32_t));
        L.take(T.part, (size_t)3 * ELMK_CONS_NPART * 3 * sizeof(double));
        L.take(T.out, 256);
      },
      [&] {  // the padding cells of down -1, then the network
        return hip_fail(ctx, hipMemsetAsync(T.down, 0xFF, (size_t)cld * sizeof(int32_t), ctx->stream), "hipMemset(runoff routing down)") ||
               upload(ctx, T.kout, kout.data(), n, "hipMemcpy(runoff routing KOUT)") || upload(ctx, T.area, area, n, "hipMemcpy(runoff routing area)") ||
               upload(ctx, T.up, up.data(), up.size(), "hipMemcpy(runoff routing up)") || upload(ctx, T.down, down, n, "hipMemcpy(runoff routing down)");
      });
}

int elmk_routing_init(elmk_ctx* ctx, const double* volr, const double* qout_sum, int64_t ncalls)
{
  const char* who = "elmk_routing_init";
  if (int rc = part_enter(ctx, BASE, who)) return rc;
  if (ncalls < 0) return invalid(ctx, "elmk_routing_init: ncalls is negative");
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = part_init(ctx, BASE, {{ROUTE_VOLR, volr}, {ROUTE_QOUT_SUM, qout_sum}})) return rc;
  if (int rc = synced(ctx)) return rc;
  ctx->route.ncalls = ncalls;
  return ELMK_OK;
}

int elmk_routing(elmk_ctx* ctx, double dt)
{
  if (int rc = part_enter(ctx, BASE, "elmk_routing")) return rc;
  if (!(dt > 0.0 && dt <= 1.0e9)) return invalid(ctx, "elmk_routing: dt must be finite and positive");
  route_launch(ctx, dt);
  ctx->route.ncalls++;
  return launched(ctx);
}

int elmk_routing_read(elmk_ctx* ctx, int which, double* host, int64_t cell0, int64_t n)
{
  const char* who = "elmk_routing_read";
  if (int rc = part_enter(ctx, BASE, who)) return rc;
  const char* why = nullptr;
  const double* const row = route_row(ctx, which, &why);
  if (!row) return invalid(ctx, "elmk_routing_read: unknown row");
  if (int rc = check_range(ctx, who, host, cell0, n, ctx->route.ncells, "cell")) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (n > 0) HIPCHK(hipMemcpyAsync(host, row + (size_t)cell0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int elmk_routing_count(elmk_ctx* ctx, int64_t* ncalls)
{
  if (int rc = part_enter(ctx, BASE, "elmk_routing_count")) return rc;
  if (!ncalls) return invalid(ctx, "elmk_routing_count: null argument");
  *ncalls = ctx->route.ncalls;
  return ELMK_OK;
}

int elmk_routing_reset_mean(elmk_ctx* ctx)
{
  if (int rc = part_enter(ctx, BASE, "elmk_routing_reset_mean")) return rc;
  Routing& T = ctx->route;
  HIPCHK(hipMemsetAsync(T.rows + ROUTE_QOUT_SUM * (size_t)T.cld, 0, (size_t)T.cld * sizeof(double), ctx->stream));
  T.ncalls = 0;
  return ELMK_OK;
}

int elmk_routing_set_withdrawal(elmk_ctx* ctx, int on)
{
  const char* who = "elmk_routing_set_withdrawal";
  if (int rc = part_enter(ctx, BASE, who)) return rc;
  if (on && !ctx->irr_rows) return invalid(ctx, "elmk_routing_set_withdrawal: the irrigation is not enabled (elmk_irrigation_enable)");
  if (!on) {
    if (int rc = irrsup_holds(ctx, who)) return rc;  // (the limit grants water that only the withdrawal takes out of VOLR)
    if (int rc = part_excludes(ctx, CMD, who)) return rc;  // (C1 forms WANT from the withdrawal)
  }
  if (int rc = refuse_capture(ctx, who)) return rc;
  ctx->route.withdraw = on != 0;  // (the captured run step is keyed by it)
  return ELMK_OK;
}

int elmk_routing_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, BASE, "elmk_routing_budget", sums); }

int elmk_routing_clear(elmk_ctx* ctx) { return part_clear(ctx, BASE, "elmk_routing_clear"); }

int elmk_routing_kinematic_enable(elmk_ctx* ctx, const double* params)
{
  const char* who = "elmk_routing_kinematic_enable";
  if (int rc = part_enter(ctx, BASE, who)) return rc;
  Routing& T = ctx->route;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_routing_kinematic_enable: the soil hydrology is not enabled (elmk_soil_hydrology_enable)");
  if (T.kw.mem) return invalid(ctx, "elmk_routing_kinematic_enable: already on");
  std::vector<double> par;
  if (int rc = invalid_map(ctx, who, kinematic_check(T.ncells, params, T.cld, &par))) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the scheme of its moment)
  const size_t cld = (size_t)T.cld;
  return part_on(
      ctx, KW,
      [&](Carve& L) {
        L.take(T.kw.rows, (size_t)KW_NROWS * cld * sizeof(double));
        L.take(T.kw.tab, (size_t)KW_NPAR * cld * sizeof(double));
      },
      [&] { return upload(ctx, T.kw.tab, par.data(), par.size(), "hipMemcpy(kinematic-wave routing parameters)"); });
}

int elmk_routing_kinematic_init(elmk_ctx* ctx, const double* wh, const double* wt)
{
  const char* who = "elmk_routing_kinematic_init";
  if (int rc = part_enter(ctx, KW, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = part_init(ctx, KW, {{KW_WH, wh}, {KW_WT, wt}})) return rc;
  return synced(ctx);
}

int elmk_routing_kinematic_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, KW, "elmk_routing_kinematic_budget", sums); }

int elmk_routing_kinematic_clear(elmk_ctx* ctx) { return part_clear(ctx, KW, "elmk_routing_kinematic_clear"); }

int elmk_routing_inundation_enable(elmk_ctx* ctx, const double* rdepth, const double* eprof)
{
  const char* who = "elmk_routing_inundation_enable";
  if (int rc = part_enter(ctx, KW, who)) return rc;
  Routing& T = ctx->route;
  if (T.fp.mem) return invalid(ctx, "elmk_routing_inundation_enable: already on");
  if (int rc = part_excludes(ctx, HEAT, who)) return rc;  // (heat on a floodplain is a later change)
  if (!rdepth || !eprof) return invalid(ctx, "elmk_routing_inundation_enable: null argument");
  int64_t cell = -1;
  const char* const text = inundation_check(T.ncells, rdepth, eprof, nullptr, nullptr, nullptr, T.cld, nullptr, &cell);
  if (int rc = invalid_at(ctx, who, text, cell)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the form of its moment)
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  // I0 reads the cells' area and the scheme's RLEN and RWIDTH: the device holds the only copies
  std::vector<double> area(n), rlen(n), rwidth(n), tab;
  if (hip_fail(ctx, hipMemcpyAsync(area.data(), T.area, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(area)") ||
      hip_fail(ctx, hipMemcpyAsync(rlen.data(), T.kw.tab + KW_RLEN * cld, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(RLEN)") ||
      hip_fail(ctx, hipMemcpyAsync(rwidth.data(), T.kw.tab + KW_RWIDTH * cld, n * 8, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpy(RWIDTH)") ||
      hip_fail(ctx, hipStreamSynchronize(ctx->stream), "hipStreamSynchronize")) {
    (void)hipStreamSynchronize(ctx->stream);
    return ELMK_E_HIP;
  }
  (void)inundation_check(T.ncells, rdepth, eprof, area.data(), rlen.data(), rwidth.data(), T.cld, &tab, nullptr);
  return part_on(
      ctx, FP,
      [&](Carve& L) {
        L.take(T.fp.rows, (size_t)FP_NROWS * cld * sizeof(double));
        L.take(T.fp.tab, (size_t)FP_NTAB * cld * sizeof(double));
      },
      [&] { return upload(ctx, T.fp.tab, tab.data(), tab.size(), "hipMemcpy(floodplain inundation tables)"); });
}

int elmk_routing_inundation_init(elmk_ctx* ctx, const double* wf)
{
  const char* who = "elmk_routing_inundation_init";
  if (int rc = part_enter(ctx, FP, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = part_init(ctx, FP, {{FP_WF, wf}})) return rc;
  return synced(ctx);
}

int elmk_routing_inundation_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, FP, "elmk_routing_inundation_budget", sums); }

int elmk_routing_inundation_clear(elmk_ctx* ctx) { return part_clear(ctx, FP, "elmk_routing_inundation_clear"); }

int elmk_routing_reservoir_enable(elmk_ctx* ctx, const double* cap, const double* target, const double* beta, const int32_t* mstart)
{
  const char* who = "elmk_routing_reservoir_enable";
  if (int rc = part_enter(ctx, KW, who)) return rc;
  Routing& T = ctx->route;
  if (T.dam.mem) return invalid(ctx, "elmk_routing_reservoir_enable: already on");
  if (int rc = part_excludes(ctx, HEAT, who)) return rc;  // (heat in a stratified reservoir is a later change)
  if (!cap || !target || !beta || !mstart) return invalid(ctx, "elmk_routing_reservoir_enable: null argument");
  std::vector<double> tab;
  std::vector<int32_t> ms;
  int64_t cell = -1;
  const char* const text = reservoir_check(T.ncells, cap, target, beta, mstart, T.cld, &tab, &ms, &cell);
  if (int rc = invalid_at(ctx, who, text, cell)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the form of its moment)
  const size_t cld = (size_t)T.cld;
  const std::vector<double> one(cld, 1.0);  // KRLS starts at 1.0, as _init leaves it
  return part_on(
      ctx, DAM,
      [&](Carve& L) {
        L.take(T.dam.rows, (size_t)DAM_NROWS * cld * sizeof(double));
        L.take(T.dam.tab, (size_t)DAM_NTAB * cld * sizeof(double));
        L.take(T.dam_mstart, cld * sizeof(int32_t));
      },
      [&] {
        return upload(ctx, T.dam.tab, tab.data(), tab.size(), "hipMemcpy(reservoir tables)") ||
               upload(ctx, T.dam_mstart, ms.data(), ms.size(), "hipMemcpy(reservoir MSTART)") ||
               upload(ctx, T.dam.rows + DAM_KRLS * cld, one.data(), cld, "hipMemcpy(reservoir KRLS)");
      });
}

int elmk_routing_reservoir_init(elmk_ctx* ctx, const double* res, const double* krls)
{
  const char* who = "elmk_routing_reservoir_init";
  if (int rc = part_enter(ctx, DAM, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  const Routing& T = ctx->route;
  const std::vector<double> one((size_t)T.cld, 1.0);
  if (int rc = part_init(ctx, DAM, {{DAM_RES, res}, {DAM_KRLS, krls}})) return rc;
  if (!krls) HIPCHK(hipMemcpyAsync(T.dam.rows + DAM_KRLS * (size_t)T.cld, one.data(), one.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);  // (`one` lives until here)
}

int elmk_routing_reservoir_time(elmk_ctx* ctx, int month, int begins)
{
  const char* who = "elmk_routing_reservoir_time";
  if (int rc = part_enter(ctx, DAM, who)) return rc;
  if (month < 0 || month > 11) return invalid(ctx, "elmk_routing_reservoir_time: month outside 0 .. 11");
  if (int rc = refuse_capture(ctx, who)) return rc;
  ctx->route.dam_time = (int32_t)(month | (begins ? 16 : 0));  // (a kernel argument of the stepwise call; the run's step reads its pad word)
  return ELMK_OK;
}

int elmk_routing_reservoir_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, DAM, "elmk_routing_reservoir_budget", sums); }

int elmk_routing_reservoir_clear(elmk_ctx* ctx) { return part_clear(ctx, DAM, "elmk_routing_reservoir_clear"); }

int elmk_routing_command_enable(elmk_ctx* ctx, const int32_t* dam, const double* share, const double* claim)
{
  const char* who = "elmk_routing_command_enable";
  if (int rc = part_enter(ctx, DAM, who)) return rc;  // (the routing, its kinematic-wave scheme, the reservoirs: each refusal says which)
  Routing& T = ctx->route;
  if (!T.withdraw) return invalid(ctx, "elmk_routing_command_enable: the routing's withdrawal is not on (elmk_routing_set_withdrawal)");
  if (T.cmd.mem) return invalid(ctx, "elmk_routing_command_enable: already on");
  if (!dam || !share || !claim) return invalid(ctx, "elmk_routing_command_enable: null argument");
  if (int rc = refuse_capture(ctx, who)) return rc;
  const size_t cld = (size_t)T.cld, n = (size_t)T.ncells;
  // the check reads CAP: the device holds the only copy
  std::vector<double> cap(n);
  HIPCHK(hipMemcpyAsync(cap.data(), T.dam.tab + DAM_CAP * cld, n * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  CommandTables C;
  int64_t cell = -1;
  const char* const text = command_check(T.ncells, cap.data(), dam, share, claim, T.cld, &C, &cell);
  if (int rc = invalid_at(ctx, who, text, cell)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the launches of its moment)
  const std::vector<double> one(cld, 1.0);
  const size_t ndams = C.dams.size(), nnz = C.tcell.size();
  T.cmd_ndams = (int64_t)ndams;
  return part_on(
      ctx, CMD,
      [&](Carve& L) {
        L.take(T.cmd.rows, (size_t)CMD_NROWS * cld * sizeof(double));
        L.take(T.cmd.tab, (size_t)2 * CMD_NDEP * cld * sizeof(double));
        L.take(T.cmd_ones, cld * sizeof(double));
        L.take(T.cmd_dam, (size_t)CMD_NDEP * cld * sizeof(int32_t));
        L.take(T.cmd_dams, (ndams + 1) * sizeof(int32_t));
        L.take(T.cmd_ptr, (ndams + 1) * sizeof(int64_t));
        L.take(T.cmd_tcell, (nnz + 1) * sizeof(int32_t));
        L.take(T.cmd_tshare, (nnz + 1) * sizeof(double));
      },
      [&] {
        return upload(ctx, T.cmd.tab, C.share.data(), C.share.size(), "hipMemcpy(command areas SHARE)") ||
               upload(ctx, T.cmd.tab + CMD_NDEP * cld, C.claim.data(), C.claim.size(), "hipMemcpy(command areas CLAIM)") ||
               upload(ctx, T.cmd_ones, one.data(), cld, "hipMemcpy(command areas ones)") ||
               upload(ctx, T.cmd.rows + CMD_RATIO * cld, one.data(), cld, "hipMemcpy(command areas RATIO)") ||
               upload(ctx, T.cmd_dam, C.dam.data(), C.dam.size(), "hipMemcpy(command areas DAM)") ||
               (ndams && upload(ctx, T.cmd_dams, C.dams.data(), ndams, "hipMemcpy(command areas dams)")) ||
               upload(ctx, T.cmd_ptr, C.ptr.data(), C.ptr.size(), "hipMemcpy(command areas ptr)") ||
               (nnz && (upload(ctx, T.cmd_tcell, C.tcell.data(), nnz, "hipMemcpy(command areas terms)") ||
                        upload(ctx, T.cmd_tshare, C.tshare.data(), nnz, "hipMemcpy(command areas terms' share)")));
      });
}

int elmk_routing_command_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, CMD, "elmk_routing_command_budget", sums); }

int elmk_routing_command_clear(elmk_ctx* ctx) { return part_clear(ctx, CMD, "elmk_routing_command_clear"); }

int elmk_routing_heat_enable(elmk_ctx* ctx, int sublev, const double* shade)
{
  const char* who = "elmk_routing_heat_enable";
  if (int rc = part_enter(ctx, KW, who)) return rc;
  Routing& T = ctx->route;
  if (T.heat.mem) return invalid(ctx, "elmk_routing_heat_enable: already on");
  if (int rc = part_excludes(ctx, FP, who)) return rc;
  if (int rc = part_excludes(ctx, DAM, who)) return rc;
  std::vector<double> ksw;
  int64_t cell = -1;
  const char* const text = heat_check(T.ncells, sublev, shade, T.cld, &ksw, &cell);
  if (int rc = invalid_at(ctx, who, text, cell)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the form of its moment)
  const size_t cld = (size_t)T.cld;
  const std::vector<double> tfrz(cld, 273.15);  // TT and TR start at TFRZ, as _init leaves them
  T.heat_sublev = sublev;
  return part_on(
      ctx, HEAT,
      [&](Carve& L) {
        L.take(T.heat.rows, (size_t)HT_NROWS * cld * sizeof(double));
        L.take(T.heat.tab, cld * sizeof(double));
      },
      [&] {
        return upload(ctx, T.heat.tab, ksw.data(), ksw.size(), "hipMemcpy(stream temperature KSW)") ||
               upload(ctx, T.heat.rows + HT_TT * cld, tfrz.data(), cld, "hipMemcpy(stream temperature TT)") ||
               upload(ctx, T.heat.rows + HT_TR * cld, tfrz.data(), cld, "hipMemcpy(stream temperature TR)");
      });
}

int elmk_routing_heat_init(elmk_ctx* ctx, const double* tt, const double* tr)
{
  const char* who = "elmk_routing_heat_init";
  if (int rc = part_enter(ctx, HEAT, who)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  const Routing& T = ctx->route;
  const std::vector<double> tfrz((size_t)T.cld, 273.15);
  if (int rc = part_init(ctx, HEAT, {{HT_TT, tt}, {HT_TR, tr}})) return rc;
  if (!tt) HIPCHK(hipMemcpyAsync(T.heat.rows + HT_TT * (size_t)T.cld, tfrz.data(), tfrz.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  if (!tr) HIPCHK(hipMemcpyAsync(T.heat.rows + HT_TR * (size_t)T.cld, tfrz.data(), tfrz.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  return synced(ctx);  // (`tfrz` lives until here)
}

int elmk_routing_heat_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, HEAT, "elmk_routing_heat_budget", sums); }

int elmk_routing_heat_clear(elmk_ctx* ctx) { return part_clear(ctx, HEAT, "elmk_routing_heat_clear"); }

int elmk_floodplain_infiltration_enable(elmk_ctx* ctx)
{
  const char* who = "elmk_floodplain_infiltration_enable";
  if (int rc = enter(ctx)) return rc;
  if (!ctx->hyd_rows) return invalid(ctx, "elmk_floodplain_infiltration_enable: the soil hydrology is not enabled (elmk_soil_hydrology_enable)");
  if (!ctx->wb_rows) return invalid(ctx, "elmk_floodplain_infiltration_enable: the water balance is not enabled (elmk_water_balance_enable)");
  if (int rc = part_enter(ctx, FP, who)) return rc;  // (the routing, its kinematic-wave scheme, the inundation: each refusal says which)
  Routing& T = ctx->route;
  if (T.land.mem) return invalid(ctx, "elmk_floodplain_infiltration_enable: already on");
  if (int rc = hs_excludes(ctx, who)) return rc;  // (the LAT and ROF forms of the hydrology kernel do not combine yet)
  if (int rc = refuse_capture(ctx, who)) return rc;
  // F0: the context keeps no host copy of the output grid's map, so from a download of its ptr and col
  const CsrMap& M = ctx->ogrid.map;
  std::vector<int64_t> ptr((size_t)M.nrows + 1);
  std::vector<int32_t> col((size_t)M.nnz), cellof;
  HIPCHK(hipMemcpyAsync(ptr.data(), M.ptr, ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (M.nnz > 0) HIPCHK(hipMemcpyAsync(col.data(), M.col, col.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  if (const int64_t shared = csr_cellof(M.nrows, ctx->ncols, ptr.data(), col.data(), &cellof); shared != -1)
    return invalid(ctx, (std::string(who) + ": column " + std::to_string(shared) +
                         " is in more than one cell of the output grid (or twice in one)").c_str());
  if (int rc = quiesce(ctx, false)) return rc;  // (the captured run step holds the forms of its moment)
  const size_t cld = (size_t)T.cld, ld = (size_t)ctx->ld;
  return part_on(
      ctx, LAND,
      [&](Carve& L) {
        L.take(T.land.rows, cld * sizeof(double));
        L.take(T.land.tab, (size_t)ELMK_FPI_NROWS * ld * sizeof(double));
        L.take(T.land_cellof, ld * sizeof(int32_t));
      },
      [&] {  // the padding columns of cellof -1, then the map's
        return hip_fail(ctx, hipMemsetAsync(T.land_cellof, 0xFF, ld * sizeof(int32_t), ctx->stream), "hipMemset(floodplain infiltration cellof)") ||
               (!cellof.empty() && upload(ctx, T.land_cellof, cellof.data(), cellof.size(), "hipMemcpy(floodplain infiltration cellof)"));
      });
}

int elmk_floodplain_infiltration_read(elmk_ctx* ctx, int which, double* host, int64_t col0, int64_t n)
{
  const char* who = "elmk_floodplain_infiltration_read";
  if (int rc = part_enter(ctx, LAND, who)) return rc;
  if (which < 0 || which >= ELMK_FPI_NROWS) return invalid(ctx, "elmk_floodplain_infiltration_read: unknown row");
  if (int rc = check_range(ctx, who, host, col0, n, ctx->ncols)) return rc;
  if (int rc = refuse_capture(ctx, who)) return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(host, ctx->route.land.tab + (size_t)which * (size_t)ctx->ld + (size_t)col0, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
  return synced(ctx);
}

int elmk_floodplain_infiltration_budget(elmk_ctx* ctx, double* sums) { return part_budget(ctx, LAND, "elmk_floodplain_infiltration_budget", sums); }

int elmk_floodplain_infiltration_clear(elmk_ctx* ctx)
{
  const char* who = "elmk_floodplain_infiltration_clear";
  if (int rc = enter(ctx)) return rc;
  if (ctx->route.land.mem && hist_has_family(ctx, ELMK_ROWS_FLOODPLAIN))
    return invalid(ctx, "elmk_floodplain_infiltration_clear: history entries over the floodplain infiltration rows exist (elmk_history_clear first)");
  if (ctx->route.land.mem)
    if (int rc = points_hold_family(ctx, who, ELMK_ROWS_FLOODPLAIN)) return rc;
  return part_clear(ctx, LAND, who);
}

}  // extern "C"
