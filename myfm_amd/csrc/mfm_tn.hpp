// mfm_tn.hpp -- the truncated standard normal samplers on a per-row Philox stream (util.hpp:15-78): the latent draws of the probit
// tasks (mfm_tasks.hpp) and of the fold-in chain (mfm_foldin_gibbs.hpp); restated draw for draw in tests/philox_ref.py.
#pragma once
#include "mfm_philox.hpp"

namespace mfm {

constexpr int TN_MAX_TRIES = 1 << 14;

// util.hpp:15-37 (Robert 2009, Prop. 2.3): z ~ N(0,1) | z > mu_minus
__device__ __forceinline__ double tn_left(RowRng &g, double mu_minus) {
  if (mu_minus < 0) {
    for (int it = 0; it < TN_MAX_TRIES; it++) {
      const double2 u = g.next2();
      const double r = sqrt(-2.0 * log(u.x));
      double s, c;
      sincospi(2.0 * u.y, &s, &c);
      if (r * c > mu_minus) return r * c;
      if (r * s > mu_minus) return r * s;
    }
    return 0.0;
  }
  const double alpha_star = (mu_minus + sqrt(mu_minus * mu_minus + 4)) / 2;
  for (int it = 0; it < TN_MAX_TRIES; it++) {
    const double2 u = g.next2();
    const double z = -log(u.x) / alpha_star + mu_minus;
    const double rho = exp(-(z - alpha_star) * (z - alpha_star) / 2);
    if (u.y < rho) return z;
  }
  return mu_minus;
}
__device__ __forceinline__ double tn_right(RowRng &g, double mu_plus) { return -tn_left(g, -mu_plus); }  // util.hpp:68-71
// util.hpp:39-60
__device__ __forceinline__ double tn_twoside(RowRng &g, double mu_minus, double mu_plus) {
  for (int it = 0; it < TN_MAX_TRIES; it++) {
    const double2 u = g.next2();
    const double z = mu_minus + (mu_plus - mu_minus) * u.x;
    double rho;
    if (mu_minus <= 0 && mu_plus >= 0)
      rho = exp(-z * z / 2);
    else if (mu_plus < 0)
      rho = exp((mu_plus * mu_plus - z * z) / 2);
    else
      rho = exp((mu_minus * mu_minus - z * z) / 2);
    if (u.y < rho) return z;
  }
  return 0.5 * (mu_minus + mu_plus);
}

}  // namespace mfm
