// mfm_pairs_ucb.hpp -- the moments form of the query x candidate scorer: mean and population standard deviation
// over the kept samples of the per-sample pair value, and the ranking value mean + beta * std. The embeddings, the selection
// buffers, the stripe lists and the merge are those of mfm_pairs.hpp, which this file leaves as it is.
//
// Per-sample value v_s(u, i): MODE 0 the score, MODE 1 Phi(score), MODE 2 sum_j Phi(score - cut_s[j]), each with the expressions of
// k_pairs_tile. The moments are Welford's recurrence in sample order,
//   d = v_s - mean;  mean += d * (1 / (s + 1));  M2 += d * (v_s - mean);      var = M2 / S,  std = sqrt(var),
// with the reciprocal rounded once per sample (exact for s + 1 a power of two). It does not cancel: a common offset of the v_s
// leaves d and M2 as they are, bitwise-equal v_s give d = 0 and so std == 0.0 exactly, and S = 1 gives M2 = v (v - v) = 0.
// (The build has -ffp-contract=off: every operation above is rounded on its own, and tests/pairs_ucb_ref.py restates them.)
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

__device__ __forceinline__ double pairs_phi(double t) { return (erf(t * 0.70710678118654752440) + 1.0) / 2.0; }

// the value of one pair under one sample from its finished score (cs: that sample's cutpoints, MODE 2)
template <int MODE>
__device__ __forceinline__ double pairs_sample_value(double t, const double *__restrict__ cs, int n_cut) {
  if constexpr (MODE == 0) {
    return t;
  } else if constexpr (MODE == 1) {
    return pairs_phi(t);
  } else {
    double v = 0.0;
    for (int j = 0; j < n_cut; j++) v += pairs_phi(t - cs[j]);
    return v;
  }
}

__device__ __forceinline__ void pairs_welford(double v, double rn, double &mean, double &m2) {
  const double d = v - mean;
  mean += d * rn;
  m2 += d * (v - mean);
}

// The tile kernel with running moments. Geometry, operand order, C/D map and the selection are k_pairs_tile's; the tile counts
// are MT * NT = 4 (32 accumulator registers and 2 x 32 of moments, against 64 + 64 of k_pairs_tile's modes 1 and 2), and every
// MODE finishes its 16 x 16 tiles per sample: KS4 k-steps, then ((w0_s + A_s[u]) + B_s[i]) + acc. The value that enters the
// selection is mean + beta * std; DENSE writes mean and std to a.dense and a.dense_std instead.
template <int MT, int NT, int MODE, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_moments(PairsArgs a) {
  typedef PairsSel<MT> L;
  constexpr int CT = 4 * NT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * L::ROWS;
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  double *buf_v = nullptr, *thr_v = nullptr;
  int *buf_i = nullptr, *thr_i = nullptr, *cnt = nullptr, *need = nullptr;
  int lim = 0;
  if constexpr (!DENSE) {
    extern __shared__ double pairs_smem[];
    buf_v = pairs_smem;
    thr_v = buf_v + L::ROWS * L::CAP;
    buf_i = (int *)(thr_v + L::ROWS);
    thr_i = buf_i + L::ROWS * L::CAP;
    cnt = thr_i + L::ROWS;
    need = cnt + L::ROWS;
    const int lim2 = 2 * a.k > 32 ? 2 * a.k : 32;
    lim = lim2 < (int)L::KP ? lim2 : (int)L::KP;
    for (int r = threadIdx.x; r < L::ROWS; r += PAIRS_WG) {
      cnt[r] = 0;
      thr_v[r] = -INFINITY;
      thr_i[r] = 2147483647;
    }
    if (threadIdx.x == 0) *need = 0;
    __syncthreads();
  }
  const double n_samples = (double)a.S;
  for (int64_t c0 = cb; c0 < ce; c0 += CT) {
    const int64_t rt0 = q0 >> 4, ct0 = (c0 >> 4) + wave * NT;
    const double *pa[MT], *pq[NT];
#pragma unroll
    for (int m = 0; m < MT; m++) pa[m] = a.Pf + (size_t)(rt0 + m) * a.NK * 64 + lane;
#pragma unroll
    for (int n = 0; n < NT; n++) pq[n] = a.Qf + (size_t)(ct0 + n) * a.NK * 64 + lane;
    double mean[MT][NT][4], m2[MT][NT][4];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int g = 0; g < 4; g++) mean[m][n][g] = m2[m][n][g] = 0.0;
    double an[MT], bn[NT];  // the next k-step's operands, loaded while this one's MFMAs run
#pragma unroll
    for (int m = 0; m < MT; m++) an[m] = a.NK > 0 ? pa[m][0] : 0.0;
#pragma unroll
    for (int n = 0; n < NT; n++) bn[n] = a.NK > 0 ? pq[n][0] : 0.0;
    int64_t ks = 0;
    for (int s = 0; s < a.S; s++) {
      pairs_d4 acc[MT][NT];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) acc[m][n] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
      for (int kk = 0; kk < a.KS4; kk++, ks++) {
        double ac[MT], bc[NT];
#pragma unroll
        for (int m = 0; m < MT; m++) ac[m] = an[m];
#pragma unroll
        for (int n = 0; n < NT; n++) bc[n] = bn[n];
        if (ks + 1 < a.NK) {
#pragma unroll
          for (int m = 0; m < MT; m++) an[m] = pa[m][(ks + 1) * 64];
#pragma unroll
          for (int n = 0; n < NT; n++) bn[n] = pq[n][(ks + 1) * 64];
        }
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
          for (int n = 0; n < NT; n++) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[m], bc[n], acc[m][n], 0, 0, 0);
      }
      const double w0 = a.w0s[s];
      const double rn = 1.0 / (double)(s + 1);
      const double *__restrict__ cs = MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr;
      double bb[NT];
#pragma unroll
      for (int n = 0; n < NT; n++) bb[n] = a.Bb[(size_t)s * a.Ipad + (ct0 + n) * 16 + (lane & 15)];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const double ab = a.Ab[(size_t)s * a.Upad + q0 + m * 16 + (lane >> 4) + 4 * g];
#pragma unroll
          for (int n = 0; n < NT; n++) {
            const double t = ((w0 + ab) + bb[n]) + acc[m][n][g];
            pairs_welford(pairs_sample_value<MODE>(t, cs, a.n_cut), rn, mean[m][n][g], m2[m][n][g]);
          }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int64_t col = (ct0 + n) * 16 + (lane & 15);
      const bool col_ok = col < ce;
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int rloc = m * 16 + (lane >> 4) + 4 * g;
          const int64_t row = q0 + rloc;
          const double sd = sqrt(m2[m][n][g] / n_samples);
          const double v = mean[m][n][g] + a.beta * sd;
          if (!col_ok || row >= a.Uc) continue;
          if (DENSE) {
            a.dense[(size_t)row * a.I + col] = mean[m][n][g];
            a.dense_std[(size_t)row * a.I + col] = sd;
          } else if (pairs_beats(v, (int)col, thr_v[rloc], thr_i[rloc])) {
            const bool excluded = a.mask && ((a.mask[(size_t)row * a.W + (col >> 5)] >> (col & 31)) & 1u);
            if (!excluded) {
              const int pos = atomicAdd(&cnt[rloc], 1);
              // (pos < CAP always, as in k_pairs_tile; the test keeps a broken invariant out of the neighbouring row's buffer)
              if (pos < L::CAP) {
                buf_v[rloc * L::CAP + pos] = v;
                buf_i[rloc * L::CAP + pos] = (int)col;
              }
              if (pos + 1 > lim) *need = 1;
            }
          }
        }
      if (!DENSE) {
        __syncthreads();
        const int go = *need;
        __syncthreads();
        if (go) {
          if (threadIdx.x == 0) *need = 0;
          pairs_compact<MT>(buf_v, buf_i, thr_v, thr_i, cnt, a.k, false);
        }
      }
    }
  }
  if (!DENSE) {
    __syncthreads();
    pairs_compact<MT>(buf_v, buf_i, thr_v, thr_i, cnt, a.k, true);
    for (int e = threadIdx.x; e < L::ROWS * a.k; e += PAIRS_WG) {
      const int row = e / a.k, j = e - row * a.k;
      const bool have = j < cnt[row];
      const size_t o = ((size_t)blockIdx.y * a.Upad + q0 + row) * a.k + j;
      a.list_v[o] = have ? buf_v[row * L::CAP + j] : -INFINITY;
      a.list_i[o] = have ? buf_i[row * L::CAP + j] : -1;
    }
  }
}

// ---- mean and std of the selected pairs ------------------------------------------------------------------------------------
// One wave per entry (query row u of the chunk, list position j) of the merged lists. The samples are taken 64 at a time: lane
// l computes v_s of sample s0 + l from the resident fragment-ordered P and Q and the per-sample biases -- the factors summed
// one after the other in factor order, which is NOT the MFMA's association, so mean + beta * std of this kernel agrees with the
// selected value within rounding, not bit for bit -- then the 64 values pass through the same Welford recurrence in sample
// order, every lane doing the same arithmetic on broadcast values. No atomics, nothing depends on the grid. An entry without a
// candidate (index -1) gets NaN for both.
template <int MODE>
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
  const double *__restrict__ P = a.Pf + (size_t)(u >> 4) * a.NK * 64 + (u & 15);
  const double *__restrict__ Q = a.Qf + (size_t)(i >> 4) * a.NK * 64 + (i & 15);
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
      const double t = ((a.w0s[s] + a.Ab[(size_t)s * a.Upad + u]) + a.Bb[(size_t)s * a.Ipad + i]) + dot;
      v = pairs_sample_value<MODE>(t, MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr, a.n_cut);
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
