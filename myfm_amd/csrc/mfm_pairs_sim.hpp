// mfm_pairs_sim.hpp -- the similarity forms of the query x candidate family: mean and population standard deviation
// over the kept samples of the per-sample cosine (or inner product) of two side rows' embeddings, and the ranking value
// mean + beta * std. Under sample s, with P_s[a, k] = sum_j V_s[k, j] a_j the embedding k_pairs_embed writes,
//   c_s(a, b) = (<P_s[a], Q_s[b]> * r_s[a]) * r_s[b],     cosine: r = 1 / sqrt(sum_k P_k^2), 0 where that sum is 0;  dot: r = 1.
// The kept samples' factors differ by signs and rotations, so an average of V means nothing, while c_s is invariant under each
// sample's own rotation: the moments are taken over the c_s. w0, w and the cutpoints play no part.
//
// Only the finish is this file's. The embedding kernels store r in the slot where the scorer's bias goes (k_pairs_embed<., ., SIM>,
// layout [S][Rpad], padding rows 0), so the finish loads the two arrays the bias finish loads; the contraction, the Welford
// accumulator (PairsWelford with this finish as its policy), the selection, the stripes, the merge and k_pairs_moments_at are the
// scorer's. Both metrics share one tile form: for the inner product the slot holds 1.0, and x * 1.0 is x. A value is not clamped.
#pragma once
#include "mfm_pairs_ucb.hpp"

namespace mfm {

// the metric of a similarity call as the C ABI numbers it (MFM_PAIRS_SIM_*), and the embedding form that serves it
constexpr int PAIRS_SIM_COSINE = 0, PAIRS_SIM_DOT = 1;

// f64 C/D map as pairs_finish_sample: lane l, register g hold (row (l >> 4) + 4 g, column l & 15) of a 16 x 16 tile.
struct PairsFinishSim {
  template <int MT, int NT, class Take>
  static __device__ __forceinline__ void tile(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT],
                                              Take take) {
    double rb[NT];
#pragma unroll
    for (int n = 0; n < NT; n++) rb[n] = a.Bb[(size_t)s * a.Ipad + (ct0 + n) * 16 + (lane & 15)];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const double ra = a.Ab[(size_t)s * a.Upad + q0 + m * 16 + (lane >> 4) + 4 * g];
#pragma unroll
        for (int n = 0; n < NT; n++) take(m, n, g, (acc[m][n][g] * ra) * rb[n]);
      }
  }
  static __device__ __forceinline__ double at(const PairsArgs &a, int s, int64_t u, int i, double dot) {
    return (dot * a.Ab[(size_t)s * a.Upad + u]) * a.Bb[(size_t)s * a.Ipad + i];
  }
};

// tile shapes and register budget: the moments forms' (MT * NT = 4)
template <int MT, int NT, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_sim(PairsArgs a) {
  pairs_tile_stripe<MT, NT, PairsWelford<MT, NT, 0, PairsFinishSim>, DENSE>(a);
}

}  // namespace mfm
