/* Host check of elmk_sin (elmkernels_amd/csrc/elmk_math.h) against the live libm's sin, bit for bit (any two NaNs count as equal).
 * gcc -O2 -mfma -ffp-contract=off -fopenmp tests/tools/sin_host_check.c -lm ; ./a.out <n per class> <seed>
 * Argument classes: 0 the physics range |x| <= 3 pi; 1 |x| <= 2e8 (from 105414350 on the
 * restated range has ended - elmk_sin returns NaN there - so that part is counted separately, not compared); 2 random bit patterns below 105414350;
 * 3 tiny and subnormal values; 4 the range boundaries of s_sin.c and their neighbours, multiples of pi/2 and specials.
 * Prints one line per class: "sin class <k> n=<evaluated> mismatches=<count>" and the first few offending arguments. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../elmkernels_amd/csrc/elmk_math.h"

static inline uint64_t mix(uint64_t z)
{
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static inline double u01(uint64_t r) { return (double)(r >> 11) * 0x1p-53; }
// outside the restated range: |x| >= 105414350 (high word 0x419921FB, where s_sin.c switches to __branred), finite
static inline int beyond_range(double x)
{
  const uint64_t b = elmk_asu64(x) & 0x7fffffffffffffffull;
  return b >= 0x419921FB00000000ull && b < 0x7ff0000000000000ull;
}
static inline int same(double a, double b)
{
  if (a != a && b != b) return 1;
  return elmk_asu64(a) == elmk_asu64(b);
}

#define NCLS 5
static const uint32_t EDGES[] = {0x3e500000u, 0x3feb6000u, 0x400368fdu, 0x419921FBu};

static double arg(int cls, long i, uint64_t seed)
{
  const uint64_t r = mix(seed * 0x100000001b3ull + (uint64_t)cls * 0x9e3779b97f4a7c15ull + (uint64_t)i);
  const double s = (r & 1) ? -1.0 : 1.0;
  switch (cls) {
    case 0: return (2.0 * u01(mix(r)) - 1.0) * 3.0 * 3.14159265358979323846;
    case 1: return (2.0 * u01(mix(r)) - 1.0) * 2.0e8;
    case 2: {
      const uint64_t b = mix(r) & 0x7fffffffffffffffull;
      const double x = elmk_asf64(b);
      return s * (beyond_range(x) ? elmk_asf64(b % 0x419921FB00000000ull) : x);
    }
    case 3: {  // subnormals, tiny normals up to 2^-20 (across the 2^-26 edge)
      const uint64_t b = mix(r) % 0x3eb0000000000000ull;
      return s * elmk_asf64(b);
    }
    default: {
      const long k = i % 64;
      if (k < 8) {
        static const double sp[8] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 0x1p-1074, 1.0, 3.14159265358979323846};
        return sp[k];
      }
      if (k < 40) {  // within +-2^16 ulps of a range boundary of s_sin.c
        const uint64_t b = ((uint64_t)EDGES[(k - 8) & 3] << 32) + (mix(r) & 0xffffu) - 0x8000u;
        return s * elmk_asf64(b);
      }
      // near a multiple of pi/2 (the reduction's hard cases), +-2^20 ulps
      const double m = (double)(mix(r) % 134217728ull) * 1.5707963267948966;
      return s * elmk_asf64(elmk_asu64(m) + (mix(r ^ 1) & 0x1fffffu) - 0x100000u);
    }
  }
}

int main(int argc, char** argv)
{
  const long n = argc > 1 ? atol(argv[1]) : 1000000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], 0, 0) : 1;
  int fail = 0;
  for (int cls = 0; cls < NCLS; cls++) {
    long bad = 0, beyond = 0;
#pragma omp parallel for reduction(+ : bad, beyond)
    for (long i = 0; i < n; i++) {
      const double x = arg(cls, i, seed);
      if (beyond_range(x)) {
        beyond++;
        continue;
      }
      bad += !same(sin(x), elmk_sin(x));
    }
    printf("sin class %d n=%ld beyond_range=%ld mismatches=%ld\n", cls, n - beyond, beyond, bad);
    if (bad) {
      int shown = 0;
      for (long i = 0; i < n && shown < 5; i++) {
        const double x = arg(cls, i, seed);
        if (beyond_range(x)) continue;
        if (!same(sin(x), elmk_sin(x))) {
          printf("  sin(%a) = %a, got %a\n", x, sin(x), elmk_sin(x));
          shown++;
        }
      }
      fail = 1;
    }
  }
  return fail;
}
