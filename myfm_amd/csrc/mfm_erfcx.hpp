// mfm_erfcx.hpp -- the scaled complementary error function erfcx(x) = exp(x^2) erfc(x), compiled for the device and the host:
// the probit latent draws (mfm_tasks.hpp) and the truncated-normal moments of the variational trainer (mfm_vb.hpp) evaluate it
// on the device, the host binding mean_var_truncated_normal_* runs the same code on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mfm {

// erfcx, same evaluation as the CPU oracle (libm erfc for small x, Laplace continued fraction beyond)
__host__ __device__ __forceinline__ double d_erfcx_pos(double x) {
  if (x < 3.0) return exp(x * x) * erfc(x);
  if (x > 5e7) return 0.5641895835477562869 / x;
  // the n-th convergent of x + (1/2)/(x + (2/2)/(x + (3/2)/(x + ...))) by the forward recurrence of its numerators and
  // denominators (all terms positive: no cancellation; x^n stays far inside the double range for these n): two FMAs per
  // level and ONE division, instead of a division per level -- in a wavefront one row in the tail makes all 64 lanes walk
  // the loop
  const int n = (x < 5) ? 90 : (x < 10 ? 50 : 25);
  double a1 = 1.0, a0 = x, b1 = 0.0, b0 = 1.0, hk = 0.0;
  for (int k = 1; k <= n; k++) {
    hk += 0.5;
    const double a = __builtin_fma(x, a0, hk * a1), b = __builtin_fma(x, b0, hk * b1);
    a1 = a0;
    a0 = a;
    b1 = b0;
    b0 = b;
  }
  return 0.5641895835477562869 * b0 / a0;
}
__host__ __device__ __forceinline__ double d_erfcx(double x) {
  if (x >= 0) return d_erfcx_pos(x);
  if (x < -26.7) return INFINITY;
  return 2 * exp(x * x) - d_erfcx_pos(-x);
}

}  // namespace mfm
