// mfm_vb.hpp -- moments of the unit-variance normal truncated to one side of 0, as the variational trainer's
// classification residual uses them (util.hpp:80-115): (mean, variance, log Z) of q(z) ~ 1{z > 0} exp(-(z - mu)^2 / 2)
// ("left") or 1{z < 0} (... ) ("right"). Compiled for the device (k_vb_score in mfm_vb.hip) and the host
// (mfm_vb_truncated_normal, bound as mean_var_truncated_normal_left / _right), so both run the same code.
#pragma once
#include "mfm_erfcx.hpp"

namespace mfm {

struct VbMoments {
  double mean, var, lnz;
};

// util.hpp:80-107: Z = 1 - Phi(-mu) scaled by 2; above 0 through erf, at or below 0 through erfcx (no underflow of Z)
__host__ __device__ inline VbMoments vb_truncnorm_left(double mu) {
  const double SQRT2 = 1.4142135623730951, SQRTPI = 1.7724538509055159;
  const double SQRT2PI = SQRT2 * SQRTPI;
  const double mu_square = mu * mu / 2;
  double phi_Z, lnZ;
  if (mu > 0) {
    const double Z = (1 - erf(-mu / SQRT2));
    phi_Z = 2 * exp(-mu_square) / SQRT2PI / Z;
    lnZ = log(Z);
  } else {
    const double Z = d_erfcx(-mu / SQRT2);
    phi_Z = 2 / Z / SQRT2PI;
    lnZ = log(Z) - mu_square;
  }
  return VbMoments{mu + phi_Z, 1 - mu * phi_Z - phi_Z * phi_Z, lnZ};
}

// util.hpp:109-115: the left form at -mu, mean negated
__host__ __device__ inline VbMoments vb_truncnorm_right(double mu) {
  VbMoments r = vb_truncnorm_left(-mu);
  r.mean = -r.mean;
  return r;
}

}  // namespace mfm
