// elmk_pair.h - two adjacent columns of a row per thread: the access shape of the row kernels (k_history.hip, k_accum.hip).
// Rows of state fields and of accumulators start at multiples of the level stride ld (a multiple of 64 columns) from 256-byte
// aligned bases, so the vector accesses are aligned, and ncols <= ld keeps the second column of a pair inside the row.
#pragma once

#include "elmk_dev.h"
#include "elmk_kernels.h"

namespace elmk {

typedef double hd2 __attribute__((ext_vector_type(2)));
typedef float hf2 __attribute__((ext_vector_type(2)));
typedef int32_t hi2 __attribute__((ext_vector_type(2)));
typedef uint32_t hu2 __attribute__((ext_vector_type(2)));
typedef uint8_t hb2 __attribute__((ext_vector_type(2)));

template <typename V> __device__ __forceinline__ V h_ld(const ELMK_GLOBAL V* p) { return __builtin_nontemporal_load(p); }
template <typename V> __device__ __forceinline__ void h_st(ELMK_GLOBAL V* p, V v) { __builtin_nontemporal_store(v, p); }

// two adjacent columns of a source row, widened to fp64 (exact for every stored type)
__device__ __forceinline__ hd2 load_pair(const void* src, int dtype, int64_t c)
{
  hd2 v;
  switch (dtype) {
    case ELMK_F64: v = h_ld((const ELMK_GLOBAL hd2*)src + c / 2); break;
    case ELMK_F32_STORED: { const hf2 f = h_ld((const ELMK_GLOBAL hf2*)src + c / 2); v = hd2{(double)f.x, (double)f.y}; break; }
    case ELMK_I32: { const hi2 i = h_ld((const ELMK_GLOBAL hi2*)src + c / 2); v = hd2{(double)i.x, (double)i.y}; break; }
    case ELMK_U32: { const hu2 u = h_ld((const ELMK_GLOBAL hu2*)src + c / 2); v = hd2{(double)u.x, (double)u.y}; break; }
    default: { const hb2 b = h_ld((const ELMK_GLOBAL hb2*)src + c / 2); v = hd2{(double)b.x, (double)b.y}; break; }
  }
  return v;
}

}  // namespace elmk
