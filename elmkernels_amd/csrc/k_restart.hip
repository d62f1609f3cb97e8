// k_restart.hip - restart images on the device (elmk_restart_save / elmk_restart_load, include/elmk.h "restart").
//
// The unit of work is a piece: a run of consecutive elements of one row (one level of one field or history accumulator) that is
// contiguous both in the device arena (lev * ld + col) and in the image ([nlev][extent], dense).  A chunk of the image is a table
// of pieces; one launch covers a chunk, grid = column blocks x pieces, so the element types are uniform across a workgroup.
//
// Every element also yields its checksum term fmix64(bits ^ fmix64(g * 64 + lev + 1)), g the global column (or output cell),
// bits the element in its image type zero-extended to 64 bits.  The terms of a workgroup are summed in LDS and written to one
// partial per workgroup with an ordinary store; k_rst_reduce sums the partials of each piece.  The sum is modulo 2^64, so the
// order of the reduction does not matter and the host adds the pieces of a section in any order.
#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

namespace {

__device__ __forceinline__ uint64_t fmix64(uint64_t k)
{
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdULL;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ULL;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ uint64_t term(uint64_t bits, int64_t g, int lev) { return fmix64(bits ^ fmix64((uint64_t)g * 64u + (uint64_t)lev + 1u)); }

// the element as stored on the device, in its image type (F64 fields widened from fp32 in the fp32-state build), as 64 bits
__device__ __forceinline__ uint64_t load_stored(const char* p, int sdtype, int64_t i)
{
  switch (sdtype) {
    case ELMK_F64: return (uint64_t)__double_as_longlong(((const double*)p)[i]);
    case ELMK_F32_STORED: return (uint64_t)__double_as_longlong((double)((const float*)p)[i]);
    case ELMK_U8: return (uint64_t)((const uint8_t*)p)[i];
    default: return (uint64_t)((const uint32_t*)p)[i];  // I32, U32: zero-extended
  }
}

__device__ __forceinline__ uint64_t load_image(const char* p, int adtype, int64_t i)
{
  switch (adtype) {
    case ELMK_F64: return ((const uint64_t*)p)[i];
    case ELMK_U8: return (uint64_t)((const uint8_t*)p)[i];
    default: return (uint64_t)((const uint32_t*)p)[i];
  }
}

__device__ __forceinline__ void store_image(char* p, int adtype, int64_t i, uint64_t v)
{
  switch (adtype) {
    case ELMK_F64: ((uint64_t*)p)[i] = v; break;
    case ELMK_U8: ((uint8_t*)p)[i] = (uint8_t)v; break;
    default: ((uint32_t*)p)[i] = (uint32_t)v; break;
  }
}

// the image element (bits of its image type) into the stored type: fp64 rounded to fp32 in the fp32-state build, as elmk_upload
__device__ __forceinline__ void store_stored(char* p, int sdtype, int64_t i, uint64_t v)
{
  switch (sdtype) {
    case ELMK_F64: ((uint64_t*)p)[i] = v; break;
    case ELMK_F32_STORED: ((float*)p)[i] = (float)__longlong_as_double((long long)v); break;
    case ELMK_U8: ((uint8_t*)p)[i] = (uint8_t)v; break;
    default: ((uint32_t*)p)[i] = (uint32_t)v; break;
  }
}

// sum of one value per thread over the workgroup (256 threads); thread 0 receives it
__device__ __forceinline__ uint64_t block_sum(uint64_t v, uint64_t* lds)
{
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  return threadIdx.x == 0 ? lds[0] + lds[1] + lds[2] + lds[3] : 0;
}

// mode 0 (save): device row -> image chunk; mode 1 (verify): image chunk only, snl range counted; mode 2 (load): image chunk -> row
template <int MODE>
__global__ __launch_bounds__(256) void k_rst_pieces(const RstPiece* __restrict__ pieces, char* __restrict__ chunk, uint64_t* __restrict__ part)
{
  __shared__ uint64_t lds[8];
  const RstPiece P = pieces[blockIdx.y];
  char* img = chunk + P.img_off;
  uint64_t sum = 0, bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < P.n; i += (int64_t)gridDim.x * 256) {
    uint64_t v;
    if (MODE == 0) {
      v = load_stored((const char*)P.dev, P.sdtype, i);
      store_image(img, P.adtype, i, v);
    } else {
      v = load_image(img, P.adtype, i);
      if (MODE == 2) store_stored((char*)P.dev, P.sdtype, i, v);
    }
    if (MODE != 2) sum += term(v, P.g0 + i, P.lev);
    if (MODE == 1 && P.snl) {
      const int32_t x = (int32_t)(uint32_t)v;
      if (x < 0 || x > NLEVSNO) bad++;
    }
  }
  if (MODE == 2) return;
  const uint64_t s = block_sum(sum, lds);
  __syncthreads();
  const uint64_t b = MODE == 1 ? block_sum(bad, lds) : 0;
  if (threadIdx.x == 0) {
    const size_t k = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[2 * k] = s;
    part[2 * k + 1] = b;
  }
}

// one thread per piece: the (checksum, out-of-range count) pairs of its nbx workgroups
__global__ __launch_bounds__(256) void k_rst_reduce(const uint64_t* __restrict__ part, int npieces, int nbx, uint64_t* __restrict__ out)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= npieces) return;
  uint64_t s = 0, b = 0;
  for (int k = 0; k < nbx; k++) {
    s += part[2 * ((size_t)p * nbx + k)];
    b += part[2 * ((size_t)p * nbx + k) + 1];
  }
  out[2 * p] = s;
  out[2 * p + 1] = b;
}

}  // namespace

void launch_restart_pieces(int mode, const RstPiece* pieces, int npieces, int nbx, char* chunk, uint64_t* part, uint64_t* sums,
                           hipStream_t st)
{
  if (npieces <= 0) return;
  const dim3 grid((unsigned)nbx, (unsigned)npieces);
  if (mode == 0)
    hipLaunchKernelGGL(k_rst_pieces<0>, grid, dim3(256), 0, st, pieces, chunk, part);
  else if (mode == 1)
    hipLaunchKernelGGL(k_rst_pieces<1>, grid, dim3(256), 0, st, pieces, chunk, part);
  else
    hipLaunchKernelGGL(k_rst_pieces<2>, grid, dim3(256), 0, st, pieces, chunk, part);
  if (mode != 2) hipLaunchKernelGGL(k_rst_reduce, dim3((unsigned)((npieces + 255) / 256)), dim3(256), 0, st, part, npieces, nbx, sums);
}

}  // namespace elmk
