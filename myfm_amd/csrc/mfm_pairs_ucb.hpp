// mfm_pairs_ucb.hpp -- the moments form of the query x candidate scorer: mean and population standard deviation
// over the kept samples of the per-sample pair value, and the ranking value mean + beta * std. Only the accumulator is this
// file's: the contraction, the samples' scores and values, the loop over a step's finished values, the selection and the
// stripe walk are the pieces of mfm_pairs.hpp (pairs_contract, pairs_finish_sample, pairs_sample_value, pairs_step, PairsSel,
// pairs_tile_stripe), the embeddings, the stripe lists and the merge its kernels.
//
// The moments are Welford's recurrence over the per-sample values v_s(u, i) (pairs_sample_value) in sample order,
//   d = v_s - mean;  mean += d * (1 / (s + 1));  M2 += d * (v_s - mean);      var = M2 / S,  std = sqrt(var),
// with the reciprocal rounded once per sample (exact for s + 1 a power of two). It does not cancel: a common offset of the v_s
// leaves d and M2 as they are, bitwise-equal v_s give d = 0 and so std == 0.0 exactly, and S = 1 gives M2 = v (v - v) = 0.
// (The build has -ffp-contract=off: every operation above is rounded on its own, and tests/pairs_ucb_ref.py restates them.)
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

__device__ __forceinline__ void pairs_welford(double v, double rn, double &mean, double &m2) {
  const double d = v - mean;
  mean += d * rn;
  m2 += d * (v - mean);
}

// The finish of the scorer's moments forms, a policy of PairsWelford and k_pairs_moments_at: the per-sample value of the pair from
// the contraction. tile: a pass's MT x NT tiles through pairs_finish_sample and pairs_sample_value; at: one pair from its inner
// product `dot`. (The similarity forms bring their own, PairsFinishSim of mfm_pairs_sim.hpp.)
template <int MODE>
struct PairsFinishScore {
  template <int MT, int NT, class Take>
  static __device__ __forceinline__ void tile(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT],
                                              Take take) {
    const double *__restrict__ cs = MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr;
    pairs_finish_sample<MT, NT>(a, s, q0, ct0, lane, acc,
                                [&](int m, int n, int g, double t) { take(m, n, g, pairs_sample_value<MODE>(t, cs, a.n_cut)); });
  }
  static __device__ __forceinline__ double at(const PairsArgs &a, int s, int64_t u, int i, double dot) {
    const double t = ((a.w0s[s] + a.Ab[(size_t)s * a.Upad + u]) + a.Bb[(size_t)s * a.Ipad + i]) + dot;
    return pairs_sample_value<MODE>(t, MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr, a.n_cut);
  }
};

// what the moments form finishes for a pair
struct PairsSpread {
  double mean, sd, v;  // v = mean + beta * sd, the ranking value
};

// The accumulator of the moments form (the interface: PairsMean). Every MODE finishes its 16 x 16 tiles per sample, and the tile
// counts are MT * NT = 4: 32 accumulator registers and 2 x 32 of moments, against 64 + 64 of the mean forms' modes 1 and 2.
// Finish: what a sample's value is (PairsFinishScore; PairsFinishSim); the recurrence, value(), store_dense and ranked are shared.
template <int MT, int NT, int MODE, class Finish = PairsFinishScore<MODE>>
struct PairsWelford {
  static constexpr bool PER_SAMPLE = true;
  typedef PairsSpread Value;
  double mean[MT][NT][4], m2[MT][NT][4];

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int g = 0; g < 4; g++) mean[m][n][g] = m2[m][n][g] = 0.0;
  }
  __device__ __forceinline__ void add(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT]) {
    const double rn = 1.0 / (double)(s + 1);
    Finish::template tile<MT, NT>(a, s, q0, ct0, lane, acc,
                                  [&](int m, int n, int g, double v) { pairs_welford(v, rn, mean[m][n][g], m2[m][n][g]); });
  }
  __device__ __forceinline__ void rows(const PairsArgs &, int64_t, int) {}
  __device__ __forceinline__ void column(const PairsArgs &, int64_t) {}
  __device__ __forceinline__ PairsSpread value(const PairsArgs &a, int m, int n, int g) const {
    const double sd = sqrt(m2[m][n][g] / (double)a.S);
    return {mean[m][n][g], sd, mean[m][n][g] + a.beta * sd};
  }
  static __device__ __forceinline__ void store_dense(const PairsArgs &a, size_t o, const PairsSpread &v) {  // two outputs
    a.dense[o] = v.mean;
    a.dense_std[o] = v.sd;
  }
  static __device__ __forceinline__ double ranked(const PairsSpread &v) { return v.v; }
};

template <int MT, int NT, int MODE, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_moments(PairsArgs a) {
  pairs_tile_stripe<MT, NT, PairsWelford<MT, NT, MODE>, DENSE>(a);
}

// ---- mean and std of the selected pairs ------------------------------------------------------------------------------------
// One wave per entry (query row u of the chunk, list position j) of the merged lists. The samples are taken 64 at a time: lane
// l computes v_s of sample s0 + l from the resident fragment-ordered P and Q and the per-sample biases -- the factors summed
// one after the other in factor order, which is NOT the MFMA's association, so mean + beta * std of this kernel agrees with the
// selected value within rounding, not bit for bit -- then the 64 values pass through the same Welford recurrence in sample
// order, every lane doing the same arithmetic on broadcast values. No atomics, nothing depends on the grid. An entry without a
// candidate (index -1) gets NaN for both. Finish::at gives the sample's value from the inner product, as Finish::tile does for a tile.
template <int MODE, class Finish = PairsFinishScore<MODE>>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_moments_at(PairsArgs a, const int32_t *__restrict__ out_i, int64_t n_entries,
                                                               double *__restrict__ out_mean, double *__restrict__ out_std) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * (PAIRS_WG / 64) + (threadIdx.x >> 6);
  if (e >= n_entries) return;
  const int64_t u = e / a.k;
  const int i = out_i[e];
  if (i < 0) {
    if (lane == 0) {
      out_mean[e] = __builtin_nan("");
      out_std[e] = __builtin_nan("");
    }
    return;
  }
  const double *__restrict__ P = a.Pf + (size_t)(u >> 4) * a.p_stride * 64 + (u & 15);
  const double *__restrict__ Q = a.Qf + (size_t)(i >> 4) * a.q_stride * 64 + (i & 15);
  const int KS = a.KS4 * 4;
  double mean = 0.0, m2 = 0.0;
  for (int s0 = 0; s0 < a.S; s0 += 64) {
    const int s = s0 + lane;
    double v = 0.0;
    if (s < a.S) {
      const size_t o = (size_t)s * a.KS4 * 64;
      double dot = 0.0;
      for (int f = 0; f < KS; f++) {
        const size_t of = o + (size_t)(f >> 2) * 64 + (f & 3) * 16;
        dot += P[of] * Q[of];
      }
      v = Finish::at(a, s, u, i, dot);
    }
    const int n_here = a.S - s0 < 64 ? a.S - s0 : 64;
    for (int j = 0; j < n_here; j++) pairs_welford(__shfl(v, j), 1.0 / (double)(s0 + j + 1), mean, m2);
  }
  if (lane == 0) {
    out_mean[e] = mean;
    out_std[e] = sqrt(m2 / (double)a.S);
  }
}

}  // namespace mfm
