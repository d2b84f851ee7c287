// mfm_pairs_vb.hpp -- the query x candidate scorer under the variational estimators' mean-field Gaussian posterior:
// mean and standard deviation of the SCORE of every pair in closed form, and the ranking value mean + beta * std. The contraction,
// the finish of a pass, the loop over a step's values, the selection and the stripe walk are the pieces of mfm_pairs.hpp, unchanged;
// this file adds the embedding of the posterior, the accumulator and the kernel for the selected pairs.
//
// A pair row a_u + b_i whose halves store disjoint columns has, per factor, the sums (M, A, B, C, E) of mfm_vb_sums.hpp of either
// half (q, c), and
//   Var[score(u, i)] = [w0_var + extra + sum x^2 wv + sum_k bracket_k](q) + [sum x^2 wv + sum_k bracket_k](c)
//                      + sum_k [ Mq^2 Ac + (Mq Aq - Bq) 2 Mc + Mq (2 Mc Ac - 2 Bc) + Aq (Mc^2 + Ac) ]_k,
// a per-query term, a per-candidate term and a dense contraction of length 4 K. It runs as FIVE pseudo-samples of width KS through
// the per-sample contraction:
//   pass 0   P = Mq, Q = Mc, w0 and the mean biases of k_pairs_embed: the finished tile is the pair's mean score, bit for bit what
//            the mean form finishes for the mean model (one sample)
//   pass 1   P = Mq^2        Q = Ac                 biases: the two per-side variance terms above, w0 = 0
//   pass 2   P = Mq Aq - Bq  Q = 2 Mc               biases 0
//   pass 3   P = Mq          Q = 2 (Mc Ac - Bc)     biases 0
//   pass 4   P = Aq          Q = Mc^2 + Ac          biases 0
// and the accumulator keeps pass 0 as the mean and adds passes 1-4, in that order, into the variance.
#pragma once
#include "mfm_pairs_ucb.hpp"
#include "mfm_vb_sums.hpp"

namespace mfm {

constexpr int PAIRS_VB_S = 5;  // pseudo-samples

// the posterior on the device: w, wv [D]; V, Vv factor-major (K, D)
struct PairsVbModel {
  const double *w, *wv, *V, *Vv;
  int64_t D;
  int K, KS;
  double var0;  // w0_var + extra_var, the query side's share
};

// A block row's share, tabulated once (the layout argument of k_pairs_embed_block): T[m][5][KS] = M, A, B, C, E per factor with the
// factors innermost, then lin[m] = sum x w, vv[m] = sum_k sum x^2 m^2, lv[m] = sum x^2 wv.
struct PairsVbBlockRef {
  const int64_t *o2b;  // [side rows], absolute side row -> block row
  const double *T, *lin, *vv, *lv;
  int64_t M;
};

// The CSR row [pb, pe) against the posterior, columns shifted by `off`: the linear mean (in the order of pairs_embed_row), the linear
// variance, and per factor f in [0, KS) the five sums handed to put(f, sums) (zeros for f >= K); sum x^2 m^2 is added to vv in the
// order of pairs_embed_row, so M and vv are that function's a and vv bit for bit.
template <class Put>
__device__ __forceinline__ void pairs_vb_row(const int32_t *__restrict__ colidx, const double *__restrict__ val, int64_t pb, int64_t pe,
                                             const PairsVbModel &mo, int64_t off, double &lin, double &lv, double &vv, Put put) {
  const double *__restrict__ w = mo.w + off, *__restrict__ wv = mo.wv + off;
  for (int64_t p = pb; p < pe; p++) lin += val[p] * w[colidx[p]];
  for (int64_t p = pb; p < pe; p++) lv += (val[p] * val[p]) * wv[colidx[p]];
  for (int f = 0; f < mo.KS; f++) {
    VbSums z;
    if (f < mo.K) {
      const double *__restrict__ Vf = mo.V + (int64_t)f * mo.D + off, *__restrict__ Sf = mo.Vv + (int64_t)f * mo.D + off;
      for (int64_t p = pb; p < pe; p++) {
        const double x = val[p], v = Vf[colidx[p]], x2 = x * x;
        vb_sums_entry(x, x2, v, Sf[colidx[p]], z.M, z.A, z.B, z.C, z.E);
        vv += x2 * (v * v);
      }
    }
    put(f, z);
  }
}

// one thread per block row m; CSR with block-local columns
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_vb_embed_block(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                   const double *__restrict__ val, int64_t M, int64_t off, PairsVbModel mo,
                                                                   double *__restrict__ T, double *__restrict__ lin_out,
                                                                   double *__restrict__ vv_out, double *__restrict__ lv_out) {
  const int64_t m = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (m >= M) return;
  double *__restrict__ Trow = T + m * 5 * mo.KS;
  const int KS = mo.KS;
  double lin = 0.0, lv = 0.0, vv = 0.0;
  pairs_vb_row(colidx, val, rowptr[m], rowptr[m + 1], mo, off, lin, lv, vv, [&](int f, const VbSums &z) {
    Trow[f] = z.M;
    Trow[KS + f] = z.A;
    Trow[2 * KS + f] = z.B;
    Trow[3 * KS + f] = z.C;
    Trow[4 * KS + f] = z.E;
  });
  lin_out[m] = lin;
  vv_out[m] = vv;
  lv_out[m] = lv;
}

// One thread per side row: the five fragment-ordered tables of the side (the layout of k_pairs_embed with S = 5: pseudo-sample s
// of row r, factor f at ((r >> 4) * 5 KS4 + s KS4 + (f >> 2)) * 64 + (f & 3) * 16 + (r & 15)) and the biases [5][Rpad]. CAND: the
// candidate side's tables, else the query side's. Summation order: the main CSR part, then -- REL -- the blocks in list order,
// as k_pairs_embed; bias 0 = lin + 1/2 (sum_k M_k^2 - vv) is that kernel's bias of the mean model. Rows [R, Rpad) are zeros.
template <bool REL, bool CAND>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_vb_embed(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                             const double *__restrict__ val, int64_t r0, int64_t R, int64_t Rpad,
                                                             PairsVbModel mo, const PairsVbBlockRef *__restrict__ blk, int n_blk,
                                                             double *__restrict__ Pf, double *__restrict__ bias) {
  const int64_t r = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (r >= Rpad) return;
  const int KS = mo.KS, KS4 = KS >> 2;
  double *__restrict__ Prow = Pf + (r >> 4) * (int64_t)(PAIRS_VB_S * KS4) * 64 + (r & 15);
  const bool live = r < R;
  int64_t pb = 0, pe = 0;
  if (live) {
    pb = rowptr[r0 + r];
    pe = rowptr[r0 + r + 1];
  }
  double lin = 0.0, lv = 0.0, vv = 0.0, sq = 0.0, br = 0.0;
  pairs_vb_row(colidx, val, pb, pe, mo, 0, lin, lv, vv, [&](int f, VbSums z) {
    if constexpr (REL) {
      if (live)
        for (int b = 0; b < n_blk; b++) {
          const double *__restrict__ t = blk[b].T + blk[b].o2b[r0 + r] * 5 * KS + f;
          z.M += t[0];
          z.A += t[KS];
          z.B += t[2 * KS];
          z.C += t[3 * KS];
          z.E += t[4 * KS];
        }
    }
    double *__restrict__ o = Prow + (int64_t)(f >> 2) * 64 + (f & 3) * 16;
    const int64_t ps = (int64_t)KS4 * 64;  // one pseudo-sample's k-steps
    const double ma_b = z.M * z.A - z.B;
    o[0] = z.M;
    if constexpr (CAND) {
      o[ps] = z.A;
      o[2 * ps] = 2.0 * z.M;
      o[3 * ps] = 2.0 * ma_b;
      o[4 * ps] = z.M * z.M + z.A;
    } else {
      o[ps] = z.M * z.M;
      o[2 * ps] = ma_b;
      o[3 * ps] = z.M;
      o[4 * ps] = z.A;
    }
    sq += z.M * z.M;
    br += vb_bracket(z.M, z.A, z.B, z.C, z.E);
  });
  if constexpr (REL) {
    if (live)
      for (int b = 0; b < n_blk; b++) {
        const int64_t e = blk[b].o2b[r0 + r];
        lin += blk[b].lin[e];
        vv += blk[b].vv[e];
        lv += blk[b].lv[e];
      }
  }
  bias[r] = lin + 0.5 * (sq - vv);
  bias[Rpad + r] = live ? ((CAND ? 0.0 : mo.var0) + lv) + br : 0.0;
  bias[2 * Rpad + r] = 0.0;
  bias[3 * Rpad + r] = 0.0;
  bias[4 * Rpad + r] = 0.0;
}

// The accumulator of the variational moments form (the interface: PairsMean). MT * NT = 4 tiles as for PairsWelford: 32 accumulator
// registers and 2 x 32 of mean and variance.
template <int MT, int NT>
struct PairsVbSpread {
  static constexpr bool PER_SAMPLE = true;
  typedef PairsSpread Value;
  double mean[MT][NT][4], var[MT][NT][4];

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++)
#pragma unroll
        for (int g = 0; g < 4; g++) mean[m][n][g] = var[m][n][g] = 0.0;
  }
  __device__ __forceinline__ void add(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT]) {
    pairs_finish_sample<MT, NT>(a, s, q0, ct0, lane, acc, [&](int m, int n, int g, double t) {
      if (s == 0)
        mean[m][n][g] = t;
      else
        var[m][n][g] += t;
    });
  }
  __device__ __forceinline__ void rows(const PairsArgs &, int64_t, int) {}
  __device__ __forceinline__ void column(const PairsArgs &, int64_t) {}
  __device__ __forceinline__ PairsSpread value(const PairsArgs &a, int m, int n, int g) const {
    const double sd = sqrt(fmax(var[m][n][g], 0.0));
    return {mean[m][n][g], sd, mean[m][n][g] + a.beta * sd};
  }
  static __device__ __forceinline__ void store_dense(const PairsArgs &a, size_t o, const PairsSpread &v) {
    a.dense[o] = v.mean;
    a.dense_std[o] = v.sd;
  }
  static __device__ __forceinline__ double ranked(const PairsSpread &v) { return v.v; }
};

template <int MT, int NT, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_vb(PairsArgs a) {
  pairs_tile_stripe<MT, NT, PairsVbSpread<MT, NT>, DENSE>(a);
}

// Mean and std of the selected pairs, the contract of k_pairs_moments_at: one thread per entry (query row u of the chunk, list
// position j) of the merged lists; the five contractions are summed factor by factor, which is not the MFMA's association, so
// mean + beta * std of this kernel agrees with the selected value within rounding (exactly where every product and sum is exact).
// An entry without a candidate (index -1) gets NaN for both.
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_vb_at(PairsArgs a, const int32_t *__restrict__ out_i, int64_t n_entries,
                                                          double *__restrict__ out_mean, double *__restrict__ out_std) {
  const int64_t e = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (e >= n_entries) return;
  const int64_t u = e / a.k;
  const int i = out_i[e];
  if (i < 0) {
    out_mean[e] = __builtin_nan("");
    out_std[e] = __builtin_nan("");
    return;
  }
  const double *__restrict__ P = a.Pf + (size_t)(u >> 4) * a.p_stride * 64 + (u & 15);
  const double *__restrict__ Q = a.Qf + (size_t)(i >> 4) * a.q_stride * 64 + (i & 15);
  const int KS = a.KS4 * 4;
  double mean = 0.0, var = 0.0;
  for (int s = 0; s < PAIRS_VB_S; s++) {
    const size_t o = (size_t)s * a.KS4 * 64;
    double dot = 0.0;
    for (int f = 0; f < KS; f++) {
      const size_t of = o + (size_t)(f >> 2) * 64 + (f & 3) * 16;
      dot += P[of] * Q[of];
    }
    const double t = ((a.w0s[s] + a.Ab[(size_t)s * a.Upad + u]) + a.Bb[(size_t)s * a.Ipad + i]) + dot;
    if (s == 0)
      mean = t;
    else
      var += t;
  }
  out_mean[e] = mean;
  out_std[e] = sqrt(fmax(var, 0.0));
}

}  // namespace mfm
