// What the two pose solvers (refine.hip's Gauss-Newton, window_ba.hip's Levenberg-Marquardt) share of a pose update: the
// index into a packed 6x6 triangle and the Rodrigues coefficients.  Both solvers are pinned to 50-digit definitions that
// form these expressions in exactly this order.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

// position of (a, b), a <= b, in the row-major upper triangle s[0..20]
__device__ __forceinline__ int tri_index(int a, int b) { return a * 6 - (a * (a - 1)) / 2 + (b - a); }

// Rodrigues coefficients sin(th)/th and (1 - cos th)/th^2: their Taylor series in th^2 for the small
// rotations an update step makes (nine terms, below 1e-17 for th < 1/4), the library functions otherwise
__device__ __forceinline__ void rodrigues_coefficients(double th2, double* a, double* b) {
  if (th2 < 0.0625) {
    double sa = 1.0, sb = 1.0;
    const double ca[8] = {1.0 / 272, 1.0 / 210, 1.0 / 156, 1.0 / 110, 1.0 / 72, 1.0 / 42, 1.0 / 20, 1.0 / 6};
    const double cb[8] = {1.0 / 306, 1.0 / 240, 1.0 / 182, 1.0 / 132, 1.0 / 90, 1.0 / 56, 1.0 / 30, 1.0 / 12};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sa = 1.0 - th2 * ca[k] * sa;
      sb = 1.0 - th2 * cb[k] * sb;
    }
    *a = sa;
    *b = 0.5 * sb;
  } else {
    const double th = sqrt(th2);
    *a = sin(th) / th;
    *b = (1.0 - cos(th)) / th2;
  }
}
