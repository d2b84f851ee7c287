// mfm_pairs.hpp -- kernels of the query x candidate scorer (mfm_pairs.hip). A pair row x = a_u + b_i whose
// halves store disjoint columns factorises:
//   score_s(u, i) = w0_s + A_s[u] + B_s[i] + sum_k P_s[u, k] Q_s[i, k],   P_s[u, k] = sum_j V_s[k, j] a_uj  (Q_s from b_i),
//   A_s[u] = w_s . a_u + 1/2 sum_k (P_s[u, k]^2 - sum_j V_s[k, j]^2 a_uj^2)                                  (B_s likewise),
// a dense (U, S KS) x (S KS, I) contraction on v_mfma_f64_16x16x4_f64 plus rank-one terms, with the per-row top-k selection
// in the contraction kernel's epilogue so that the (U, I) matrix is never written. A side may carry relation blocks (row r
// additionally holds row o2b[r] of a block): their share of P_s, of the linear term and of sum V^2 x^2 is tabulated once per block row
// and gathered (k_pairs_embed_block / k_pairs_embed). Values: the mean over the samples of the score, of Phi(score), or -- ordered
// probit -- of sum_j Phi(score - cut_s[j]), the expected class index.
//
// Every form of the tile kernel -- the mean forms here, the moments form (mfm_pairs_ucb.hpp), the rank form (mfm_pairs_rank.hpp),
// the per-sample selecting form (mfm_pairs_samples.hpp) -- is put together from the pieces of this file, each of which exists once:
//   pairs_contract        the MFMA contraction of one workgroup step, pass by pass
//   pairs_finish_sample   a pass's tile -> the samples' scores ((w0 + A) + B) + acc;  pairs_sample_value: score -> value
//   PairsMean             the accumulator of the mean forms (PairsWelford, the moments form's, is in mfm_pairs_ucb.hpp)
//   pairs_step            contraction + accumulator + the guarded loop over the step's finished values
//   PairsSel              the per-row selection (LDS state, push, compaction round, list write)
//   pairs_select_stripe   the selecting workgroup: a row tile of P x a stripe of candidates into the stripe's lists
//   pairs_tile_stripe     a dense or selecting workgroup over its stripe, for either accumulator
// so a value finished by one form is bit for bit the value another form finishes for that pair (the build does not contract
// a * b + c).
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
// The CSR row [pb, pe) times w and V, the one loop of the three embedding kernels: returns the linear term, hands put(f, a_f) the
// row's factor f for every f in [0, KS) (zero for f >= K) and adds sum_j V[f, j]^2 x_j^2 over the factors to vv, all in CSR
// order. V is read where it lies (factor-major (K, D), the store's layout): a side's rows hold a few entries each, and
// neighbouring one-hot rows gather neighbouring columns. Without SIDE_TERMS (the similarity embedding, mfm_pairs_sim.hpp) only the
// factors are formed: w is not read, neither the linear term nor vv is summed, the returned value is 0.
template <bool SIDE_TERMS = true, class Put>
__device__ __forceinline__ double pairs_embed_row(const int32_t *__restrict__ colidx, const double *__restrict__ val, int64_t pb,
                                                  int64_t pe, const double *__restrict__ w, const double *__restrict__ V, int64_t D,
                                                  int K, int KS, double &vv, Put put) {
  double lin = 0.0;
  if constexpr (SIDE_TERMS)
    for (int64_t p = pb; p < pe; p++) lin += val[p] * w[colidx[p]];
  for (int f = 0; f < KS; f++) {
    double a = 0.0;
    if (f < K) {
      const double *__restrict__ Vf = V + (int64_t)f * D;
      for (int64_t p = pb; p < pe; p++) {
        const double x = val[p], v = Vf[colidx[p]];
        a += x * v;
        if constexpr (SIDE_TERMS) vv += (x * x) * (v * v);
      }
    }
    put(f, a);
  }
  return lin;
}

// A side row is [main | B_0[o2b_0[r]] | B_1[o2b_1[r]] ...]: what a block row adds to P, to the linear term and to sum V^2 x^2 does not
// depend on the side row that points at it, so it is computed once per block row (k_pairs_embed_block) and gathered per side row
// (k_pairs_embed<true>): O(K * blocks) per side row instead of O(K * nnz of the expanded row).
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
// SIM (the similarity embedding): the factors alone, lin and vv are neither computed nor written.
template <bool SIM = false>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_embed_block(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                                const double *__restrict__ val, int64_t M, int64_t off,
                                                                const double *const *__restrict__ wv, int64_t D, int K, int KS,
                                                                double *__restrict__ T, double *__restrict__ lin_out,
                                                                double *__restrict__ vv_out) {
  const int64_t m = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (m >= M) return;
  const int s = blockIdx.y;
  double *__restrict__ Trow = T + ((int64_t)s * M + m) * KS;
  double vv = 0.0;
  const double lin = pairs_embed_row<!SIM>(colidx, val, rowptr[m], rowptr[m + 1], wv[s] + off, wv[s] + D + off, D, K, KS, vv,
                                           [&](int f, double a) { Trow[f] = a; });
  if constexpr (!SIM) {
    lin_out[(int64_t)s * M + m] = lin;
    vv_out[(int64_t)s * M + m] = vv;
  }
}

// One thread per (side row, sample): P_s[r, 0..KS) in the order the MFMA reads it and the bias A_s[r]. Fragment order: the 64
// values of (16-row tile t, k-step q) -- q counts groups of 4 factors through all samples, q = s KS/4 + k/4 -- are contiguous,
// value (row r, factor k) at (k & 3) * 16 + (r & 15): lane l of v_mfma_f64_16x16x4_f64 holds A[row l & 15][k l >> 4] (and
// B[k l >> 4][col l & 15]), so a wave's operand load is 512 contiguous bytes. Rows [R, Rpad) and factors [K, KS) are written as
// zeros (the tables hold zeros for k >= K).
// Summation order, fixed: the main CSR part, then -- REL, a side with relation blocks -- the blocks in list order (block b adds
// T_b[s][o2b_b[r0 + r]][.] to P, lin_b to lin, vv_b to vv), then bias = lin + 1/2 (sum_k P_k^2 - vv). o2b is indexed with the
// ABSOLUTE side row r0 + r: a query chunk does not re-base it. Without REL neither blk nor n_blk is read.
// MAPPED (the row -> sample plan of mfm_pairs_samples.hpp): output row r holds side row r0 + map_row[r] (-1: a padding row, zeros)
// under sample map_s[r] alone -- one thread per output row, P with KS / 4 k-steps per row tile and one bias per row, the
// arithmetic of a row under its sample unchanged. Without MAPPED neither map is read.
// SIM (the similarity forms, mfm_pairs_sim.hpp): the bias slot holds the row's normalisation r instead -- SIM 1
// (cosine) r = 1 / sqrt(sq) with sq = sum_k P_k^2 summed in factor order as above, r = 0 where sq is 0 (an empty row, rank 0, an
// all-zero embedding; an sq that overflowed gives 0 as well, and the value of such a row may be NaN: finite embeddings are
// assumed); SIM 2 (dot) r = 1 -- and 0 for a padding row; neither w nor a block's lin / vv is read. SIM 0 is the scorer's
// embedding, unchanged.
template <bool REL, bool MAPPED = false, int SIM = 0>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_embed(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                          const double *__restrict__ val, int64_t r0, int64_t R, int64_t Rpad,
                                                          const double *const *__restrict__ wv, int64_t D, int K, int KS, int S,
                                                          const PairsBlockRef *__restrict__ blk, int n_blk,
                                                          double *__restrict__ Pf, double *__restrict__ bias,
                                                          const int32_t *__restrict__ map_row, const int32_t *__restrict__ map_s) {
  const int64_t r = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (r >= Rpad) return;
  const int s = MAPPED ? map_s[r] : (int)blockIdx.y;
  const double *__restrict__ w = wv[s];
  const int KS4 = KS >> 2;
  const int64_t NK = MAPPED ? (int64_t)KS4 : (int64_t)S * KS4;
  double *__restrict__ Prow = Pf + ((r >> 4) * NK + (MAPPED ? (int64_t)0 : (int64_t)s * KS4)) * 64 + (r & 15);
  const int64_t src = MAPPED ? (int64_t)map_row[r] : r;  // the side row, relative to r0
  const bool live = MAPPED ? src >= 0 : r < R;
  int64_t pb = 0, pe = 0;
  if (live) {
    pb = rowptr[r0 + src];
    pe = rowptr[r0 + src + 1];
  }
  double sq = 0.0, vv = 0.0;
  double lin = pairs_embed_row<SIM == 0>(colidx, val, pb, pe, w, w + D, D, K, KS, vv, [&](int f, double a) {
    if constexpr (REL) {
      if (live)
        for (int b = 0; b < n_blk; b++) a += blk[b].T[((int64_t)s * blk[b].M + blk[b].o2b[r0 + src]) * KS + f];
    }
    Prow[(int64_t)(f >> 2) * 64 + (f & 3) * 16] = a;
    sq += a * a;
  });
  if constexpr (REL && SIM == 0) {
    if (live)
      for (int b = 0; b < n_blk; b++) {
        const int64_t e = (int64_t)s * blk[b].M + blk[b].o2b[r0 + src];
        lin += blk[b].lin[e];
        vv += blk[b].vv[e];
      }
  }
  if constexpr (SIM == 0)
    bias[(MAPPED ? (int64_t)0 : (int64_t)s * Rpad) + r] = lin + 0.5 * (sq - vv);
  else
    bias[(MAPPED ? (int64_t)0 : (int64_t)s * Rpad) + r] = !live ? 0.0 : SIM == 2 ? 1.0 : sq > 0.0 ? 1.0 / sqrt(sq) : 0.0;
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

// ---- the tile kernels' argument ------------------------------------------------------------------------------------------
struct PairsPlanEntry;  // (mfm_pairs_samples.hpp)

struct PairsArgs {
  // the contraction
  const double *Pf, *Qf;                    // fragment-ordered embeddings: [rows / 16][p_stride or q_stride][64]
  int64_t NK;                               // k-steps the contraction walks: S * KS4
  int64_t p_stride, q_stride;               // k-steps between two row tiles of P and of Q (NK, but for a one-sample view of more)
  int KS4, S;
  // the finish of a value
  const double *Ab, *Asum, *Bb, *Bsum;      // biases: [S][Upad], [Upad], [S][Ipad], [Ipad]
  const double *w0s;                        // [S]
  double w0sum;
  const double *cut;                        // [S][n_cut]: the samples' cutpoints (MODE 2)
  int n_cut;
  double beta;                              // the moments form ranks by mean + beta * std
  // the grid's share of the pairs
  int64_t Upad, Ipad, Uc, I;                // the chunk's padded / valid query rows, the padded / valid candidates
  int64_t stripe_len;                       // candidates per stripe, a multiple of the workgroup step
  // dense forms
  double *dense;                            // [Uc][I]: the value (the moments form: the mean)
  double *dense_std;                        // [Uc][I]: the moments form's second output
  // selecting forms
  const uint32_t *mask;                     // [Uc][W] or null: the exclusions (the counting rank form reads it too)
  int64_t W;
  int k;
  double *list_v;                           // [stripes][Upad][k]: each stripe's best k per row, in order, padded (-inf, -1)
  int32_t *list_i;
  // rank form (mfm_pairs_rank.hpp)
  const int64_t *tptr;                      // the targets: CSR over ALL query rows, indexed u0 + row
  const int32_t *tidx;
  double *tval;                             // [the chunk's targets]: entry tptr[u0 + row] - tbase + t, the target's value
  int32_t *trank;                           // [the chunk's targets]: its rank, zeroed per chunk
  int64_t u0, tbase;                        // the chunk's first query row and tptr[u0]
  // per-sample selecting form (mfm_pairs_samples.hpp)
  const PairsPlanEntry *plan;               // the launch's entries, one per blockIdx.x
  const int32_t *row_of;                    // [P rows] or null: the chunk's query row of a row of P (the row -> sample plan)
  int64_t list_rows;                        // rows of one stripe's lists
};

// ---- the contraction -------------------------------------------------------------------------------------------------------
// A workgroup owns MT * 16 query rows (from q0) and walks candidates in steps of 4 * NT * 16; wave w accumulates the MT x NT tiles
// of 16 x 16 pairs at candidate tiles [ct0, ct0 + NT), ct0 = step / 16 + w NT. The k-steps are walked in passes -- PER_SAMPLE: S
// passes of KS4, one sample's factors each; else one pass of all NK -- and after each pass done(s, acc) gets the finished
// acc[MT][NT]. The next k-step's operands are loaded while this one's MFMAs run, across pass boundaries too.
template <int MT, int NT, bool PER_SAMPLE, class Done>
__device__ __forceinline__ void pairs_contract(const PairsArgs &a, int64_t q0, int64_t ct0, int lane, Done done) {
  const int64_t rt0 = q0 >> 4;
  const double *pa[MT], *pq[NT];
#pragma unroll
  for (int m = 0; m < MT; m++) pa[m] = a.Pf + (size_t)(rt0 + m) * a.p_stride * 64 + lane;
#pragma unroll
  for (int n = 0; n < NT; n++) pq[n] = a.Qf + (size_t)(ct0 + n) * a.q_stride * 64 + lane;
  double an[MT], bn[NT];
#pragma unroll
  for (int m = 0; m < MT; m++) an[m] = a.NK > 0 ? pa[m][0] : 0.0;
#pragma unroll
  for (int n = 0; n < NT; n++) bn[n] = a.NK > 0 ? pq[n][0] : 0.0;
  const int n_pass = PER_SAMPLE ? a.S : 1;
  const int64_t per_pass = PER_SAMPLE ? (int64_t)a.KS4 : a.NK;
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
      // the k-step's MFMAs issue before the wait for the next step's operands: without this the scheduler may pull the
      // next step's an -> ac copies, and with them that wait, up between the MFMAs (seen in the (1, 8) selecting form, + 6 %)
      __builtin_amdgcn_sched_barrier(0);
    }
    done(s, acc);
  }
}

// f64 C/D map: lane l, register g hold (row (l >> 4) + 4 g, column l & 15) of a 16 x 16 tile.
// The scores of sample s from its pass's acc, ((w0_s + A_s[u]) + B_s[i]) + acc in that association: take(m, n, g, score).
template <int MT, int NT, class Take>
__device__ __forceinline__ void pairs_finish_sample(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane,
                                                    const pairs_d4 (&acc)[MT][NT], Take take) {
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
      for (int n = 0; n < NT; n++) take(m, n, g, ((w0 + ab) + bb[n]) + acc[m][n][g]);
    }
}

__device__ __forceinline__ double pairs_phi(double t) { return (erf(t * 0.70710678118654752440) + 1.0) / 2.0; }

// the value of one pair under one sample from its score (cs: that sample's cutpoints, MODE 2): MODE 0 the score, MODE 1 Phi(score),
// MODE 2 (ordered probit) sum_{j < n_cut} Phi(score - cut[s][j]) = sum_c c p_c, the expected class index under that sample's class
// probabilities (P(y > j) = Phi(score - cut_j))
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

// ---- the accumulator of the mean forms ---------------------------------------------------------------------------------------
// An accumulator takes the passes of one workgroup step (zero, add) and then gives the step's values, column by column
// (rows once, column(col) per tile column, value(m, n, g)); store_dense and ranked say what a dense form writes of a value and
// what a selecting form ranks by.
// The mean. MODE 0: all samples are one inner dimension, the summed biases and the summed w0 are added once:
// ((w0sum + Asum[u]) + Bsum[i]) + acc, over S. MODES 1, 2: the samples' values summed in sample order in registers, over S.
template <int MT, int NT, int MODE>
struct PairsMean {
  static constexpr bool PER_SAMPLE = MODE != 0;
  typedef double Value;
  pairs_d4 tot[MT][NT];
  double asum[MT][4], bsum;

  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++) tot[m][n] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
  }
  __device__ __forceinline__ void add(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT]) {
    if constexpr (MODE == 0) {
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++) tot[m][n] = acc[m][n];
    } else {
      const double *__restrict__ cs = MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr;
      pairs_finish_sample<MT, NT>(a, s, q0, ct0, lane, acc, [&](int m, int n, int g, double t) {
        if constexpr (MODE == 2) {
          // term by term onto the running total, NOT tot += pairs_sample_value<2>(t): that sums the sample's terms from zero
          // first, another association and so other bits than every release so far
          for (int j = 0; j < a.n_cut; j++) tot[m][n][g] += pairs_phi(t - cs[j]);
        } else {
          tot[m][n][g] += pairs_sample_value<MODE>(t, cs, a.n_cut);
        }
      });
    }
  }
  __device__ __forceinline__ void rows(const PairsArgs &a, int64_t q0, int lane) {
    if constexpr (MODE == 0) {
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) asum[m][g] = a.w0sum + a.Asum[q0 + m * 16 + (lane >> 4) + 4 * g];
    }
  }
  __device__ __forceinline__ void column(const PairsArgs &a, int64_t col) { bsum = MODE == 0 ? a.Bsum[col] : 0.0; }
  __device__ __forceinline__ double value(const PairsArgs &a, int m, int n, int g) const {
    const double inv_div = (double)a.S;
    return MODE == 0 ? ((asum[m][g] + bsum) + tot[m][n][g]) / inv_div : tot[m][n][g] / inv_div;
  }
  static __device__ __forceinline__ void store_dense(const PairsArgs &a, size_t o, double v) { a.dense[o] = v; }  // one output
  static __device__ __forceinline__ double ranked(double v) { return v; }
};

// ---- one workgroup step ----------------------------------------------------------------------------------------------------
// Contraction of the step at candidate c0 into an Acc, then the loop over the finished values, written once for every form: tile
// column by tile column (a round: one tile column per wave), put(rloc, row, col, value) for the pairs inside the chunk and the
// stripe [., ce), and round() after each tile column, reached by all threads.
template <int MT, int NT, class Acc, class Put, class Round>
__device__ __forceinline__ void pairs_step(const PairsArgs &a, int64_t q0, int64_t c0, int64_t ce, Put put, Round round) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t ct0 = (c0 >> 4) + wave * NT;
  Acc sum;
  sum.zero();
  pairs_contract<MT, NT, Acc::PER_SAMPLE>(a, q0, ct0, lane, [&](int s, const pairs_d4(&acc)[MT][NT]) { sum.add(a, s, q0, ct0, lane, acc); });
  sum.rows(a, q0, lane);
#pragma unroll
  for (int n = 0; n < NT; n++) {
    const int64_t col = (ct0 + n) * 16 + (lane & 15);
    const bool col_ok = col < ce;
    sum.column(a, col);
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int rloc = m * 16 + (lane >> 4) + 4 * g;
        const int64_t row = q0 + rloc;
        const typename Acc::Value v = sum.value(a, m, n, g);
        if (!col_ok || row >= a.Uc) continue;
        put(rloc, row, col, v);
      }
    round();
  }
}

// ---- the selection -----------------------------------------------------------------------------------------------------------
// LDS of a selecting workgroup: per query row a buffer of CAP candidates that survived the row's threshold, its fill count and
// the threshold (the row's k-th best at the last compaction; (-inf, INT_MAX) = take everything until k are known)
template <int MT>
struct PairsSel {
  static constexpr int ROWS = MT * 16;
  static constexpr int KP = 256 / MT;   // the largest k this tile shape serves
  static constexpr int CAP = KP + 64;   // one round appends at most 64 per row (4 waves x 16 columns)
  static constexpr int EPL = CAP / 64;  // buffer entries per lane when a wave compacts a row
  static constexpr size_t BYTES = (size_t)ROWS * CAP * 12 + (size_t)ROWS * 16 + 16;

  double *buf_v, *thr_v;
  int *buf_i, *thr_i, *cnt, *need;
  int k, lim;  // a fill beyond lim asks for a compaction before the next round

  __device__ __forceinline__ void init(int k_) {
    extern __shared__ double pairs_smem[];
    buf_v = pairs_smem;
    thr_v = buf_v + ROWS * CAP;
    buf_i = (int *)(thr_v + ROWS);
    thr_i = buf_i + ROWS * CAP;
    cnt = thr_i + ROWS;
    need = cnt + ROWS;
    k = k_;
    const int lim2 = 2 * k > 32 ? 2 * k : 32;
    lim = lim2 < (int)KP ? lim2 : (int)KP;
    for (int r = threadIdx.x; r < ROWS; r += PAIRS_WG) {
      cnt[r] = 0;
      thr_v[r] = -INFINITY;
      thr_i[r] = 2147483647;
    }
    if (threadIdx.x == 0) *need = 0;
    __syncthreads();
  }

  // a finished value: the threshold first (most values end here), then the exclusion mask, then the row's buffer
  __device__ __forceinline__ void push(const PairsArgs &a, int rloc, int64_t row, int64_t col, double v) {
    if (!pairs_beats(v, (int)col, thr_v[rloc], thr_i[rloc])) return;
    const bool excluded = a.mask && ((a.mask[(size_t)row * a.W + (col >> 5)] >> (col & 31)) & 1u);
    if (excluded) return;
    const int pos = atomicAdd(&cnt[rloc], 1);
    // (cnt <= KP before a round and a round appends at most 64 per row, so pos < CAP always; the test keeps a
    //  broken invariant from writing into the neighbouring row's buffer)
    if (pos < CAP) {
      buf_v[rloc * CAP + pos] = v;
      buf_i[rloc * CAP + pos] = (int)col;
    }
    if (pos + 1 > lim) *need = 1;
  }

  // Sorts the buffers of the rows with at least k entries (final: of every row) into the total order, keeps the best k and sets
  // the threshold. A row belongs to ONE wave: every lane ranks its entries against the whole buffer (all reads), then the
  // entries of rank < k are written at their rank -- the wave runs in lockstep and n is uniform, so no read follows a write.
  __device__ __forceinline__ void compact(bool final) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int row = wave; row < ROWS; row += PAIRS_WG / 64) {
      const int n = cnt[row] < (int)CAP ? cnt[row] : (int)CAP;
      if (n == 0 || (!final && n < k)) continue;
      double *bv = buf_v + row * CAP;
      int *bi = buf_i + row * CAP;
      double ev[EPL];
      int ei[EPL], rk[EPL];
#pragma unroll
      for (int t = 0; t < EPL; t++) {
        const int e = lane + 64 * t;
        ev[t] = e < n ? bv[e] : 0.0;
        ei[t] = e < n ? bi[e] : 0;
        rk[t] = 0;
      }
      for (int j = 0; j < n; j++) {
        const double vj = bv[j];
        const int ij = bi[j];
#pragma unroll
        for (int t = 0; t < EPL; t++) rk[t] += pairs_beats(vj, ij, ev[t], ei[t]) ? 1 : 0;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int t = 0; t < EPL; t++) {
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

  // after a round (one tile column per wave), by all threads: compact when some row's fill asked for it
  __device__ __forceinline__ void round() {
    __syncthreads();
    const int go = *need;
    __syncthreads();
    if (go) {
      if (threadIdx.x == 0) *need = 0;
      compact(false);
    }
  }

  // the stripe's list of every row of the tile, from list row q0 on: its best k in order, padded (-inf, -1)
  __device__ __forceinline__ void finish(const PairsArgs &a, int64_t q0) {
    __syncthreads();
    compact(true);
    for (int e = threadIdx.x; e < ROWS * k; e += PAIRS_WG) {
      const int row = e / k, j = e - row * k;
      const bool have = j < cnt[row];
      const size_t o = ((size_t)blockIdx.y * a.list_rows + q0 + row) * k + j;
      a.list_v[o] = have ? buf_v[row * CAP + j] : -INFINITY;
      a.list_i[o] = have ? buf_i[row * CAP + j] : -1;
    }
  }
};

// ---- the dense and the selecting forms -----------------------------------------------------------------------------------------
// The selecting workgroup: the MT * 16 rows of P from q0 against the stripe [cb, ce), Acc::ranked of the values through the per-row
// selection, the stripe's lists written at list row l0. mask_row(row): the row of the exclusion mask that belongs to a row of P.
template <int MT, int NT, class Acc, class MaskRow>
__device__ __forceinline__ void pairs_select_stripe(const PairsArgs &a, int64_t q0, int64_t l0, int64_t cb, int64_t ce, MaskRow mask_row) {
  PairsSel<MT> sel;
  sel.init(a.k);
  for (int64_t c0 = cb; c0 < ce; c0 += 4 * NT * 16)
    pairs_step<MT, NT, Acc>(
        a, q0, c0, ce,
        [&](int rloc, int64_t row, int64_t col, const typename Acc::Value &v) { sel.push(a, rloc, mask_row(row), col, Acc::ranked(v)); },
        [&] { sel.round(); });
  sel.finish(a, l0);
}

// A workgroup over its MT * 16 query rows x one stripe of candidates, for either accumulator. DENSE writes every value
// (Acc::store_dense; it asks for no LDS and sets none up); otherwise the selecting workgroup.
template <int MT, int NT, class Acc, bool DENSE>
__device__ __forceinline__ void pairs_tile_stripe(const PairsArgs &a) {
  const int64_t q0 = (int64_t)blockIdx.x * (MT * 16);
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  if constexpr (DENSE) {
    for (int64_t c0 = cb; c0 < ce; c0 += 4 * NT * 16)
      pairs_step<MT, NT, Acc>(
          a, q0, c0, ce, [&](int, int64_t row, int64_t col, const typename Acc::Value &v) { Acc::store_dense(a, (size_t)row * a.I + col, v); },
          [] {});
  } else {
    pairs_select_stripe<MT, NT, Acc>(a, q0, q0, cb, ce, [](int64_t row) { return row; });
  }
}

// the mean forms: MODE 0 the score, 1 Phi(score), 2 the ordered probit's expected class index
template <int MT, int NT, int MODE, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile(PairsArgs a) {
  pairs_tile_stripe<MT, NT, PairsMean<MT, NT, MODE>, DENSE>(a);
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
