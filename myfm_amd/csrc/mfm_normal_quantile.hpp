// mfm_normal_quantile.hpp -- Phi^-1 on the host, the one definition of the binding (_myfm.cpp: the root bracket of the device's
// mixture solve) and of the library (mfm_ess.hpp: the table of rank-normalised values).
#pragma once
#include <cmath>

// Phi^-1(p), 0 < p < 1, by bisection of 0.5 erfc(-z / sqrt 2) down to neighbouring doubles
inline double mfm_std_normal_quantile(double p) {
  double lo = -40.0, hi = 40.0;
  for (int it = 0; it < 200; it++) {
    const double mid = 0.5 * (lo + hi);
    if (!(mid > lo && mid < hi)) break;
    if (0.5 * std::erfc(-mid * 0.70710678118654752440) < p)
      lo = mid;
    else
      hi = mid;
  }
  return 0.5 * (lo + hi);
}
