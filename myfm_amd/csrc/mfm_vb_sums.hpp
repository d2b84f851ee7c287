// mfm_vb_sums.hpp -- the five sums of the score's variance under a mean-field Gaussian posterior, the one statement of
// them that the row pass (mfm_vbmoments.hpp) and the pair scorer (mfm_pairs_vb.hpp) share.
//
// Posterior V_jk ~ N(m_jk, s_jk), independent. For one factor and a row with entries x_j write t_j = x_j m_j, g_j = x_j^2 s_j:
//   M = sum t     A = sum g     B = sum g t     C = sum (g t) t     E = sum g g
// and the factor's share of Var[score] is
//   M^2 A - 2 M B + C + 1/2 (A^2 - E)  =  sum_i g_i (M - t_i)^2 + sum_{i<j} g_i g_j  >= 0,
// evaluated as  (M (M A - B) - (M B - C)) + 1/2 (A A - E):  for a row with ONE entry M A and B are the same product, M B and C are
// the same product and A A and E are the same product, so the share is 0.0 exactly and not a rounding residue of either sign.
// All five sums are additive over the parts of a row (main table, relation blocks), which is what lets a block row's share be
// tabulated once.
#pragma once

namespace mfm {

struct VbSums {
  double M = 0.0, A = 0.0, B = 0.0, C = 0.0, E = 0.0;
};

// one entry (x, x2 = x * x) of the row against the factor's posterior mean m and variance s
__device__ __forceinline__ void vb_sums_entry(double x, double x2, double m, double s, double &M, double &A, double &B, double &C,
                                              double &E) {
  const double t = x * m, g = x2 * s, gt = g * t;
  M += t;
  A += g;
  B += gt;
  C += gt * t;
  E += g * g;
}

__device__ __forceinline__ double vb_bracket(double M, double A, double B, double C, double E) {
  return (M * (M * A - B) - (M * B - C)) + 0.5 * (A * A - E);
}

}  // namespace mfm
