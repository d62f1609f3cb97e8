// k_solar.hip - the solar lines of kokkos_init_timestep (init_timestep_kokkos.cc:26-34) for every column of the context, each at
// its own latitude and longitude (elmk_solar_geometry).  The reference computes one average_cosz / daylength / max_daylength for
// the whole domain on the host ("only one value currently", :27); here every column gets the reference's bits for its own
// location.  What is the same for all columns comes in as kernel arguments, what does not change with time was computed once
// on the host (DevState::geo), and the rest is elmk_solar_column (elmk_solar.h): two acos and four sin per column.
// Bytes per column: 7 x 8 read, 3 x 8 written (coszen, dayl, dayl_factor).
//
// Shortwave in COSZEN mode (elmk_set_shortwave_mode) also needs czf, the mean cos(zenith) over the forcing record's interval:
// elmk_solar_avg_cosz at the record's scalars (forc_dt, rec_decday).  Stepwise, k_forcing_cosz writes it from the geography rows;
// in elmk_run, k_solar_geometry_run_cz writes it beside coszen from the row it already holds (one acos, four sin, 8 bytes more).
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_solar.h"

namespace elmk {

// one column of one step: the body of k_solar_geometry and of its run-mode variants; CZ: also czf[c] at the record's scalars q
template <bool CZ = false>
__device__ __forceinline__ void solar_geometry_col(const DevState* __restrict__ S, int64_t c, const elmk_solar_step& p,
                                                   const elmk_solar_step* q = nullptr, double* __restrict__ czf = nullptr)
{
  const int64_t ld = S->ld;
  double g[ELMK_GEO_N];
#pragma unroll
  for (int k = 0; k < ELMK_GEO_N; k++) g[k] = S->geo[(int64_t)k * ld + c];
  double cosz, dayl, dayl_factor;
  elmk_solar_column(g, &p, &cosz, &dayl, &dayl_factor);
  S->coszen[c] = cosz;
  S->col_dayl[(int64_t)COL_DAYL * ld + c] = dayl;
  S->col_dayl[(int64_t)COL_DAYL_FACTOR * ld + c] = dayl_factor;
  if (CZ) czf[c] = elmk_solar_avg_cosz(g, q);
}

__global__ __launch_bounds__(256) void k_solar_geometry(const DevState* __restrict__ S, const elmk_solar_step p)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S->ncols) return;
  solar_geometry_col(S, c, p);
}

// elmk_run: the step's scalars from its row of the step table
__global__ __launch_bounds__(256) void k_solar_geometry_run(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                            const int32_t* __restrict__ cursor)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S->ncols) return;
  const elmk_solar_step p = rows[*cursor].sol;
  solar_geometry_col(S, c, p);
}

// elmk_run in COSZEN mode: also czf of the step's forcing record, from the record-time table (one row per forcing slot)
__global__ __launch_bounds__(256) void k_solar_geometry_run_cz(const DevState* __restrict__ S, const RunRow* __restrict__ rows,
                                                               const int32_t* __restrict__ cursor, const elmk_solar_step* __restrict__ rec,
                                                               double* __restrict__ czf)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S->ncols) return;
  const RunRow* __restrict__ r = rows + *cursor;
  const elmk_solar_step p = r->sol, q = rec[r->forc_slot];
  solar_geometry_col<true>(S, c, p, &q, czf);
}

// elmk_set_forcing_record_time: czf of every column at the record's scalars q
__global__ __launch_bounds__(256) void k_forcing_cosz(const DevState* __restrict__ S, const elmk_solar_step q, double* __restrict__ czf)
{
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= S->ncols) return;
  const int64_t ld = S->ld;
  double g[ELMK_GEO_N];
#pragma unroll
  for (int k = 0; k <= ELMK_GEO_COS_LAT; k++) g[k] = S->geo[(int64_t)k * ld + c];
  czf[c] = elmk_solar_avg_cosz(g, &q);
}

void launch_solar_geometry(const DevState* S, int64_t n, const elmk_solar_step& p, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_solar_geometry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, p);
}

void launch_solar_geometry_run(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_solar_geometry_run, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, rows, cursor);
}

void launch_solar_geometry_run_cz(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, const elmk_solar_step* rec,
                                  double* czf, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_solar_geometry_run_cz, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, rows, cursor, rec, czf);
}

void launch_forcing_cosz(const DevState* S, int64_t n, const elmk_solar_step& q, double* czf, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_forcing_cosz, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, q, czf);
}

}  // namespace elmk
