// k_solar.hip - the solar lines of kokkos_init_timestep (init_timestep_kokkos.cc:26-34) for every column of the context, each at
// its own latitude and longitude (elmk_solar_geometry).  The reference computes one average_cosz / daylength / max_daylength for
// the whole domain on the host ("only one value currently", :27); here every column gets the reference's bits for its own
// location.  What is the same for all columns comes in as kernel arguments, what does not change with time was computed once
// on the host (DevState::geo), and the rest is elmk_solar_column (elmk_solar.h): two acos and four sin per column.
// Bytes per column: 7 x 8 read, 3 x 8 written (coszen, dayl, dayl_factor).
#include "elmk_dev.h"
#include "elmk_kernels.h"
#include "elmk_solar.h"

namespace elmk {

// one column of one step: the body of k_solar_geometry and of its run-mode variant
__device__ __forceinline__ void solar_geometry_col(const DevState* __restrict__ S, int64_t c, const elmk_solar_step& p)
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

void launch_solar_geometry(const DevState* S, int64_t n, const elmk_solar_step& p, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_solar_geometry, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, p);
}

void launch_solar_geometry_run(const DevState* S, int64_t n, const RunRow* rows, const int32_t* cursor, hipStream_t st)
{
  if (n > 0) hipLaunchKernelGGL(k_solar_geometry_run, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S, rows, cursor);
}

}  // namespace elmk
