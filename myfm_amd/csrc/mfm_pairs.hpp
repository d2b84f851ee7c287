// mfm_pairs.hpp -- kernels of the query x candidate scorer (mfm_pairs.hip). A pair row x = a_u + b_i whose
// halves store disjoint columns factorises:
//   score_s(u, i) = w0_s + A_s[u] + B_s[i] + sum_k P_s[u, k] Q_s[i, k],   P_s[u, k] = sum_j V_s[k, j] a_uj  (Q_s from b_i),
//   A_s[u] = w_s . a_u + 1/2 sum_k (P_s[u, k]^2 - sum_j V_s[k, j]^2 a_uj^2)                                  (B_s likewise),
// a dense (U, S KS) x (S KS, I) contraction on v_mfma_f64_16x16x4_f64 plus rank-one terms, with the per-row top-k selection
// in the contraction kernel's epilogue so that the (U, I) matrix is never written. A side may carry relation blocks (row r
// additionally holds row o2b[r] of a block): their share of P_s, of the linear term and of sum V^2 x^2 is tabulated once per block row
// and gathered (k_pairs_embed_block / k_pairs_embed_rel). Values: the mean over the samples of the score, of Phi(score), or -- ordered
// probit -- of sum_j Phi(score - cut_s[j]), the expected class index.
#pragma once
#include "mfm_common.hpp"

namespace mfm {

constexpr int PAIRS_WG = 256;        // 4 waves: the same query rows, side-by-side candidate columns
constexpr int PAIRS_ROW_ALIGN = 64;  // query chunks are padded to the largest workgroup tile (zero rows)
constexpr int PAIRS_COL_ALIGN = 512; // candidates are padded to the widest workgroup step (zero rows)
constexpr int PAIRS_MAX_K = 256;
constexpr int PAIRS_MAX_STRIPES = 64;

typedef double pairs_d4 __attribute__((ext_vector_type(4)));

// the total order of the selection: value descending, candidate index ascending
__device__ __forceinline__ bool pairs_beats(double va, int ia, double vb, int ib) { return va > vb || (va == vb && ia < ib); }

// ---- side embedding ----------------------------------------------------------------------------------------------------
// One thread per (row, sample): P_s[r, 0..KS) in the order the MFMA reads it and the bias A_s[r]. Fragment order: the 64
// values of (16-row tile t, k-step q) -- q counts groups of 4 factors through all samples, q = s KS/4 + k/4 -- are contiguous,
// value (row r, factor k) at (k & 3) * 16 + (r & 15): lane l of v_mfma_f64_16x16x4_f64 holds A[row l & 15][k l >> 4] (and
// B[k l >> 4][col l & 15]), so a wave's operand load is 512 contiguous bytes. V is read where it lies (factor-major (K, D), the
// store's layout): a side's rows hold a few entries each, and neighbouring one-hot rows gather neighbouring columns. Rows
// [R, Rpad) and factors [K, KS) are written as zeros.
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_embed(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                          const double *__restrict__ val, int64_t r0, int64_t R, int64_t Rpad,
                                                          const double *const *__restrict__ wv, int64_t D, int K, int KS,
                                                          int S, double *__restrict__ Pf, double *__restrict__ bias) {
  const int64_t r = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (r >= Rpad) return;
  const int s = blockIdx.y;
  const double *__restrict__ w = wv[s];
  const double *__restrict__ V = w + D;
  const int KS4 = KS >> 2;
  const int64_t NK = (int64_t)S * KS4;
  double *__restrict__ Prow = Pf + ((r >> 4) * NK + (int64_t)s * KS4) * 64 + (r & 15);
  int64_t pb = 0, pe = 0;
  if (r < R) {
    pb = rowptr[r0 + r];
    pe = rowptr[r0 + r + 1];
  }
  double lin = 0.0, sq = 0.0, vv = 0.0;
  for (int64_t p = pb; p < pe; p++) lin += val[p] * w[colidx[p]];
  for (int f = 0; f < KS; f++) {
    double a = 0.0;
    if (f < K) {
      const double *__restrict__ Vf = V + (int64_t)f * D;
      for (int64_t p = pb; p < pe; p++) {
        const double x = val[p], v = Vf[colidx[p]];
        a += x * v;
        vv += (x * x) * (v * v);
      }
    }
    Prow[(int64_t)(f >> 2) * 64 + (f & 3) * 16] = a;
    sq += a * a;
  }
  bias[(int64_t)s * Rpad + r] = lin + 0.5 * (sq - vv);
}

// ---- side embedding with relation blocks ---------------------------------------------------------------------------------
// A side row is [main | B_0[o2b_0[r]] | B_1[o2b_1[r]] ...]: what a block row adds to P, to the linear term and to sum V^2 x^2 does not
// depend on the side row that points at it, so it is computed once per block row (k_pairs_embed_block) and gathered per side row
// (k_pairs_embed_rel): O(K * blocks) per side row instead of O(K * nnz of the expanded row).
//
// Table layout of one block of M rows, one allocation of S * M * (KS + 2) doubles:
//   T[(s * M + m) * KS + k] = sum_j V_s[k, off + j] x_mj  (zero for k in [K, KS)),   then lin[s * M + m] = sum_j w_s[off + j] x_mj,
//   then vv[s * M + m] = sum_k sum_j V_s[k, off + j]^2 x_mj^2.
// Row-major in m with the KS factors innermost: the gathering thread owns one (side row, sample) and walks the factors, so its KS
// reads of a block row are one contiguous run (whole cache lines: KS * 8 is a multiple of 32 bytes), and side rows that share a block
// row -- the common case, many ratings per user -- read the same lines. A fragment-ordered table would scatter them 128 bytes apart.
// lin and vv are read once per (side row, sample) and stay out of the T rows so that those keep their alignment.
struct PairsBlockRef {
  const int64_t *o2b;  // [side rows], absolute side row -> block row
  const double *T, *lin, *vv;
  int64_t M;
};

// One thread per (block row m, sample s). CSR with block-local columns; `off`: the block's first column in the model's feature space.
// V is read factor-major where it lies, as k_pairs_embed does.
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_embed_block(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                const double *__restrict__ val, int64_t M, int64_t off,
                                                                const double *const *__restrict__ wv, int64_t D, int K, int KS,
                                                                double *__restrict__ T, double *__restrict__ lin_out,
                                                                double *__restrict__ vv_out) {
  const int64_t m = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (m >= M) return;
  const int s = blockIdx.y;
  const double *__restrict__ w = wv[s] + off;
  const double *__restrict__ V = wv[s] + D + off;
  const int64_t pb = rowptr[m], pe = rowptr[m + 1];
  double *__restrict__ Trow = T + ((int64_t)s * M + m) * KS;
  double lin = 0.0, vv = 0.0;
  for (int64_t p = pb; p < pe; p++) lin += val[p] * w[colidx[p]];
  for (int f = 0; f < KS; f++) {
    double a = 0.0;
    if (f < K) {
      const double *__restrict__ Vf = V + (int64_t)f * D;
      for (int64_t p = pb; p < pe; p++) {
        const double x = val[p], v = Vf[colidx[p]];
        a += x * v;
        vv += (x * x) * (v * v);
      }
    }
    Trow[f] = a;
  }
  lin_out[(int64_t)s * M + m] = lin;
  vv_out[(int64_t)s * M + m] = vv;
}

// One thread per (side row, sample), grid and row padding of k_pairs_embed. Summation order, fixed: the main CSR part exactly as
// k_pairs_embed forms it, then the blocks in list order (block b adds T_b[s][o2b_b[r0 + r]][.] to P, lin_b to lin, vv_b to vv), then
// bias = lin + 1/2 (sum_k P_k^2 - vv). o2b is indexed with the ABSOLUTE side row r0 + r: a query chunk does not re-base it. P in
// fragment order; rows [R, Rpad) and factors [K, KS) are zeros (the tables hold zeros for k >= K).
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_embed_rel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                              const double *__restrict__ val, int64_t r0, int64_t R, int64_t Rpad,
                                                              const double *const *__restrict__ wv, int64_t D, int K, int KS, int S,
                                                              const PairsBlockRef *__restrict__ blk, int n_blk,
                                                              double *__restrict__ Pf, double *__restrict__ bias) {
  const int64_t r = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (r >= Rpad) return;
  const int s = blockIdx.y;
  const double *__restrict__ w = wv[s];
  const double *__restrict__ V = w + D;
  const int KS4 = KS >> 2;
  const int64_t NK = (int64_t)S * KS4;
  double *__restrict__ Prow = Pf + ((r >> 4) * NK + (int64_t)s * KS4) * 64 + (r & 15);
  const bool live = r < R;
  int64_t pb = 0, pe = 0;
  if (live) {
    pb = rowptr[r0 + r];
    pe = rowptr[r0 + r + 1];
  }
  double lin = 0.0, sq = 0.0, vv = 0.0;
  for (int64_t p = pb; p < pe; p++) lin += val[p] * w[colidx[p]];
  for (int f = 0; f < KS; f++) {
    double a = 0.0;
    if (f < K) {
      const double *__restrict__ Vf = V + (int64_t)f * D;
      for (int64_t p = pb; p < pe; p++) {
        const double x = val[p], v = Vf[colidx[p]];
        a += x * v;
        vv += (x * x) * (v * v);
      }
    }
    if (live)
      for (int b = 0; b < n_blk; b++) a += blk[b].T[((int64_t)s * blk[b].M + blk[b].o2b[r0 + r]) * KS + f];
    Prow[(int64_t)(f >> 2) * 64 + (f & 3) * 16] = a;
    sq += a * a;
  }
  if (live)
    for (int b = 0; b < n_blk; b++) {
      const int64_t e = (int64_t)s * blk[b].M + blk[b].o2b[r0 + r];
      lin += blk[b].lin[e];
      vv += blk[b].vv[e];
    }
  bias[(int64_t)s * Rpad + r] = lin + 0.5 * (sq - vv);
}

// sum over the samples, in sample order, of a side's biases (regression mode adds it once)
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_bias_sum(const double *__restrict__ bias, int S, int64_t Rpad,
                                                             double *__restrict__ out) {
  const int64_t r = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (r >= Rpad) return;
  double t = 0.0;
  for (int s = 0; s < S; s++) t += bias[(int64_t)s * Rpad + r];
  out[r] = t;
}

// exclusion bitmask of a query chunk: bit (u - u0, i) set for every stored (u, i); one wave per query row
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_mask(const int64_t *__restrict__ eptr, const int32_t *__restrict__ eidx,
                                                         int64_t u0, int64_t Uc, int64_t W, uint32_t *__restrict__ mask) {
  const int64_t u = (int64_t)blockIdx.x * (PAIRS_WG / 64) + (threadIdx.x >> 6);
  if (u >= Uc) return;
  const int64_t pe = eptr[u0 + u + 1];
  for (int64_t p = eptr[u0 + u] + (threadIdx.x & 63); p < pe; p += 64) {
    const int32_t c = eidx[p];
    atomicOr(&mask[u * W + (c >> 5)], 1u << (c & 31));
  }
}

// ---- contraction with fused selection ----------------------------------------------------------------------------------
struct PairsArgs {
  const double *Pf, *Qf;                    // fragment-ordered embeddings: [rows / 16][NK][64]
  const double *Ab, *Asum, *Bb, *Bsum;      // biases: [S][Upad], [Upad], [S][Ipad], [Ipad]
  const double *w0s;                        // [S]
  double w0sum;
  int64_t NK;                               // k-steps through all samples: S * KS4
  int KS4, S;
  int64_t Upad, Ipad, Uc, I;                // the chunk's padded / valid query rows, the padded / valid candidates
  int64_t stripe_len;                       // candidates per stripe, a multiple of the workgroup step
  const uint32_t *mask;                     // [Uc][W] or null
  int64_t W;
  int k;
  double *list_v;                           // [stripes][Upad][k]: each stripe's best k per row, in order, padded (-inf, -1)
  int32_t *list_i;
  double *dense;                            // [Uc][I] (the scores entry points)
  const double *cut;                        // [S][n_cut]: the samples' cutpoints (MODE 2; last, so that the other modes' argument
  int n_cut;                                //  offsets are what they were)
  double *dense_std;                        // [Uc][I]: the moments form's second dense output (mfm_pairs_ucb.hpp; dense holds the mean)
  double beta;                              // the moments form ranks by mean + beta * std (last, for the same reason)
  const int64_t *tptr;                      // the rank form's targets (mfm_pairs_rank.hpp): CSR over ALL query rows, indexed u0 + row
  const int32_t *tidx;
  double *tval;                             // [the chunk's targets]: entry tptr[u0 + row] - tbase + t, the target's value
  int32_t *trank;                           // [the chunk's targets]: its rank, zeroed per chunk
  int64_t u0, tbase;                        // the chunk's first query row and tptr[u0]
};

// LDS of the selecting kernel: per query row a buffer of CAP candidates that survived the row's threshold, its fill count and
// the threshold (the row's k-th best at the last compaction; (-inf, INT_MAX) = take everything until k are known)
template <int MT>
struct PairsSel {
  static constexpr int ROWS = MT * 16;
  static constexpr int KP = 256 / MT;   // the largest k this tile shape serves
  static constexpr int CAP = KP + 64;   // one round appends at most 64 per row (4 waves x 16 columns)
  static constexpr int EPL = CAP / 64;  // buffer entries per lane when a wave compacts a row
  static constexpr size_t BYTES = (size_t)ROWS * CAP * 12 + (size_t)ROWS * 16 + 16;
};

// Sorts the buffers of the rows with at least k entries (final: of every row) into the total order, keeps the best k and sets
// the threshold. A row belongs to ONE wave: every lane ranks its entries against the whole buffer (all reads), then the
// entries of rank < k are written at their rank -- the wave runs in lockstep and n is uniform, so no read follows a write.
template <int MT>
__device__ __forceinline__ void pairs_compact(double *buf_v, int *buf_i, double *thr_v, int *thr_i, int *cnt, int k, bool final) {
  typedef PairsSel<MT> L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int row = wave; row < L::ROWS; row += PAIRS_WG / 64) {
    const int n = cnt[row] < (int)L::CAP ? cnt[row] : (int)L::CAP;
    if (n == 0 || (!final && n < k)) continue;
    double *bv = buf_v + row * L::CAP;
    int *bi = buf_i + row * L::CAP;
    double ev[L::EPL];
    int ei[L::EPL], rk[L::EPL];
#pragma unroll
    for (int t = 0; t < L::EPL; t++) {
      const int e = lane + 64 * t;
      ev[t] = e < n ? bv[e] : 0.0;
      ei[t] = e < n ? bi[e] : 0;
      rk[t] = 0;
    }
    for (int j = 0; j < n; j++) {
      const double vj = bv[j];
      const int ij = bi[j];
#pragma unroll
      for (int t = 0; t < L::EPL; t++) rk[t] += pairs_beats(vj, ij, ev[t], ei[t]) ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < L::EPL; t++) {
      const int e = lane + 64 * t;
      if (e < n && rk[t] < k) {
        bv[rk[t]] = ev[t];
        bi[rk[t]] = ei[t];
        if (rk[t] == k - 1) {
          thr_v[row] = ev[t];
          thr_i[row] = ei[t];
        }
      }
    }
    if (lane == 0) cnt[row] = n < k ? n : k;
  }
  __syncthreads();
}

// A workgroup owns MT * 16 query rows x one stripe of candidates and walks the stripe in steps of 4 * NT * 16 candidates; wave w
// accumulates the MT x NT tiles of 16 x 16 pairs at candidate tiles [w NT, (w + 1) NT) of the step. f64 C/D map: lane l, register
// g hold (row (l >> 4) + 4 g, column l & 15). MODE 0: all samples are one inner dimension of NK k-steps, the mean biases and the
// mean w0 are added once. MODE 1: a tile is finished per sample (KS4 k-steps), Phi applied, and summed in sample order in
// registers. MODE 2 (ordered probit): as MODE 1, but a sample adds sum_{j < n_cut} Phi(score - cut[s][j]) = sum_c c p_c, the expected
// class index under that sample's class probabilities (P(y > j) = Phi(score - cut_j)). DENSE writes the tile; otherwise the values go through the per-row selection (rounds of one tile column per wave).
template <int MT, int NT, int MODE, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile(PairsArgs a) {
  typedef PairsSel<MT> L;
  constexpr int CT = 4 * NT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * L::ROWS;
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  // the selection's LDS (the dense form asks for none and sets none of this up)
  double *buf_v = nullptr, *thr_v = nullptr;
  int *buf_i = nullptr, *thr_i = nullptr, *cnt = nullptr, *need = nullptr;
  int lim = 0;  // a fill beyond it asks for a compaction before the next round
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
  const double inv_div = (double)a.S;
  for (int64_t c0 = cb; c0 < ce; c0 += CT) {
    const int64_t rt0 = q0 >> 4, ct0 = (c0 >> 4) + wave * NT;
    const double *pa[MT], *pq[NT];
#pragma unroll
    for (int m = 0; m < MT; m++) pa[m] = a.Pf + (size_t)(rt0 + m) * a.NK * 64 + lane;
#pragma unroll
    for (int n = 0; n < NT; n++) pq[n] = a.Qf + (size_t)(ct0 + n) * a.NK * 64 + lane;
    pairs_d4 tot[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++) tot[m][n] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
    double an[MT], bn[NT];  // the next k-step's operands, loaded while this one's MFMAs run
#pragma unroll
    for (int m = 0; m < MT; m++) an[m] = a.NK > 0 ? pa[m][0] : 0.0;
#pragma unroll
    for (int n = 0; n < NT; n++) bn[n] = a.NK > 0 ? pq[n][0] : 0.0;
    const int n_pass = MODE != 0 ? a.S : 1;
    const int64_t per_pass = MODE != 0 ? (int64_t)a.KS4 : a.NK;
    int64_t ks = 0;
    for (int s = 0; s < n_pass; s++) {
      pairs_d4 acc[MT][NT];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) acc[m][n] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
      for (int64_t kk = 0; kk < per_pass; kk++, ks++) {
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
      if (MODE != 0) {
        const double w0 = a.w0s[s];
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
              if constexpr (MODE == 2) {
                const double *__restrict__ cs = a.cut + (size_t)s * a.n_cut;
                for (int j = 0; j < a.n_cut; j++) tot[m][n][g] += (erf((t - cs[j]) * 0.70710678118654752440) + 1.0) / 2.0;
              } else {
                tot[m][n][g] += (erf(t * 0.70710678118654752440) + 1.0) / 2.0;
              }
            }
          }
      } else {
#pragma unroll
        for (int m = 0; m < MT; m++)
#pragma unroll
          for (int n = 0; n < NT; n++) tot[m][n] = acc[m][n];
      }
    }
    double asum[MT][4];
    if (MODE == 0) {
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) asum[m][g] = a.w0sum + a.Asum[q0 + m * 16 + (lane >> 4) + 4 * g];
    }
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int64_t col = (ct0 + n) * 16 + (lane & 15);
      const bool col_ok = col < ce;
      const double bsum = MODE == 0 ? a.Bsum[col] : 0.0;
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int rloc = m * 16 + (lane >> 4) + 4 * g;
          const int64_t row = q0 + rloc;
          const double v = MODE == 0 ? ((asum[m][g] + bsum) + tot[m][n][g]) / inv_div : tot[m][n][g] / inv_div;
          if (!col_ok || row >= a.Uc) continue;
          if (DENSE) {
            a.dense[(size_t)row * a.I + col] = v;
          } else if (pairs_beats(v, (int)col, thr_v[rloc], thr_i[rloc])) {
            const bool excluded = a.mask && ((a.mask[(size_t)row * a.W + (col >> 5)] >> (col & 31)) & 1u);
            if (!excluded) {
              const int pos = atomicAdd(&cnt[rloc], 1);
              // (cnt <= KP before a round and a round appends at most 64 per row, so pos < CAP always; the test keeps a
              //  broken invariant from writing into the neighbouring row's buffer)
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

// ---- merge: the stripes' lists of one query row into its final k under the same order (one workgroup per row) -------------
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_merge(const double *__restrict__ list_v, const int32_t *__restrict__ list_i,
                                                          int n_stripes, int64_t Upad, int k, double *__restrict__ out_v,
                                                          int32_t *__restrict__ out_i) {
  const int64_t u = blockIdx.x;
  for (int j = threadIdx.x; j < k; j += PAIRS_WG) {
    out_v[u * k + j] = -INFINITY;
    out_i[u * k + j] = -1;
  }
  __syncthreads();
  const int n = n_stripes * k;
  for (int e = threadIdx.x; e < n; e += PAIRS_WG) {
    const size_t oe = ((size_t)(e / k) * Upad + u) * k + (e % k);
    const int ie = list_i[oe];
    if (ie < 0) continue;
    const double ve = list_v[oe];
    int rank = 0;
    for (int st = 0; st < n_stripes && rank < k; st++) {
      const size_t o = ((size_t)st * Upad + u) * k;
      for (int j = 0; j < k; j++) {
        const int ij = list_i[o + j];
        if (ij < 0 || !pairs_beats(list_v[o + j], ij, ve, ie)) break;  // (a stripe's list is in order: the rest loses too)
        rank++;
      }
    }
    if (rank < k) {
      out_v[u * k + rank] = ve;
      out_i[u * k + rank] = ie;
    }
  }
}

}  // namespace mfm
