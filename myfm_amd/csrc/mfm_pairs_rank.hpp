// mfm_pairs_rank.hpp -- ranks of given (query, candidate) pairs among all candidates of their query. The rank of
// a target pair is the number of admissible candidates (valid, not excluded, not the target itself) that beat it under the total
// order of the selection, pairs_beats: value descending, candidate index ascending. It is an exact integer count, independent of
// tiles, stripes and chunks. The embeddings, the exclusion mask and the stripes are those of mfm_pairs.hpp, which this file leaves
// as it is.
//
// Two passes of one kernel over the same fragment-ordered P and Q, both with the value expression of k_pairs_tile word for word
// (the build does not contract a * b + c, so a value finished here is bit for bit the one the dense and the selecting form finish
// for that pair):
//   COUNT = false  the values at the targets: a finished value looks its column up in its row's target list and on a hit stores
//                  itself to tval. Only the candidate steps that hold a target of the row tile are walked.
//   COUNT = true   the ranks: the targets' values are the thresholds; a finished value at an admissible column adds one to the LDS
//                  counter of every target of its row that it beats. Counters go to global memory with integer atomics at the end
//                  of the stripe: the sum does not depend on the grid or on the order of the additions.
// Targets come as a CSR pattern with sorted, unique columns and at most PAIRS_RANK_MAX_T entries per query row.
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

constexpr int PAIRS_RANK_MAX_T = 64;  // targets of one query row per call
constexpr int PAIRS_RANK_ROWS = 64;   // the one tile shape, (MT, NT) = (4, 2): 64 query rows x 128 candidates per step

// LDS per workgroup: the target columns of its 64 rows and their counts, a word for workgroup-wide decisions; the counting form
// adds the targets' values, the counters and per row its weakest target (the one every other target of the row beats)
template <bool COUNT>
struct PairsRankLds {
  static constexpr int N = PAIRS_RANK_ROWS * PAIRS_RANK_MAX_T;
  static constexpr size_t BYTES = (COUNT ? (size_t)N * 8 + PAIRS_RANK_ROWS * 8 : 0) + (size_t)N * 4 + PAIRS_RANK_ROWS * 4 + 16 +
                                  (COUNT ? (size_t)N * 4 + PAIRS_RANK_ROWS * 4 : 0);
};

template <int MT, int NT, int MODE, bool COUNT>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_rank(PairsArgs a) {
  static_assert(MT * 16 == PAIRS_RANK_ROWS, "the target lists are laid out for 64 query rows");
  constexpr int ROWS = MT * 16, TMAX = PAIRS_RANK_MAX_T, NL = ROWS * TMAX;
  constexpr int CT = 4 * NT * 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * ROWS;
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  extern __shared__ double pairs_rank_smem[];
  double *tv = nullptr, *weak_v = nullptr;  // COUNT: [ROWS][TMAX] thresholds, [ROWS] the weakest
  int *cnt = nullptr, *weak_i = nullptr;    // COUNT: [ROWS][TMAX] counters
  int *ti, *tn, *word;                      // [ROWS][TMAX] target columns, [ROWS] their number, the workgroup's word
  if constexpr (COUNT) {
    tv = pairs_rank_smem;
    weak_v = tv + NL;
    ti = (int *)(weak_v + ROWS);
  } else {
    ti = (int *)pairs_rank_smem;
  }
  tn = ti + NL;
  word = tn + ROWS;
  if constexpr (COUNT) {
    cnt = word + 4;
    weak_i = cnt + NL;
  }
  // ---- the row tile's targets (rows past the chunk have none)
  if (threadIdx.x == 0) word[0] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < NL; e += PAIRS_WG) {
    const int r = e / TMAX, t = e - r * TMAX;
    const int64_t row = q0 + r;
    int64_t pb = 0, pe = 0;
    if (row < a.Uc) {
      pb = a.tptr[a.u0 + row];
      pe = a.tptr[a.u0 + row + 1];
    }
    const int n = (int)(pe - pb) < TMAX ? (int)(pe - pb) : TMAX;
    if (t == 0) {
      tn[r] = n;
      if (n > 0) word[0] = 1;
    }
    if (t < n) {
      ti[e] = a.tidx[pb + t];
      if constexpr (COUNT) tv[e] = a.tval[pb - a.tbase + t];
    }
    if constexpr (COUNT) cnt[e] = 0;
  }
  __syncthreads();
  if (word[0] == 0) return;  // a row tile without targets has nothing to find and nothing to count
  if constexpr (COUNT) {
    // (+inf, -1) loses to nothing: a row without targets counts nothing
    for (int r = threadIdx.x; r < ROWS; r += PAIRS_WG) {
      double wv = INFINITY;
      int wi = -1;
      for (int t = 0; t < tn[r]; t++)
        if (t == 0 || pairs_beats(wv, wi, tv[r * TMAX + t], ti[r * TMAX + t])) {
          wv = tv[r * TMAX + t];
          wi = ti[r * TMAX + t];
        }
      weak_v[r] = wv;
      weak_i[r] = wi;
    }
  }
  __syncthreads();
  int cur = 0;  // COUNT = false, threads [0, ROWS): the first target of the thread's row at or after the step under way
  const double inv_div = (double)a.S;
  for (int64_t c0 = cb; c0 < ce; c0 += CT) {
    if constexpr (!COUNT) {
      // jump to the next step of the stripe that holds a target of this row tile
      if (threadIdx.x == 0) word[1] = 2147483647;
      __syncthreads();
      if (threadIdx.x < ROWS) {
        const int r = threadIdx.x, n = tn[r];
        while (cur < n && ti[r * TMAX + cur] < c0) cur++;
        if (cur < n) atomicMin(&word[1], ti[r * TMAX + cur]);
      }
      __syncthreads();
      const int64_t nx = word[1];
      __syncthreads();
      if (nx >= ce) break;
      c0 = cb + (nx - cb) / CT * CT;
    }
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
          const int nt = tn[rloc];
          const int *__restrict__ trow = ti + rloc * TMAX;
          if constexpr (!COUNT) {
            // the column's place in the row's sorted target list, if it has one
            int lo = 0, hi = nt;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (trow[mid] < (int)col)
                lo = mid + 1;
              else
                hi = mid;
            }
            if (lo < nt && trow[lo] == (int)col) a.tval[a.tptr[a.u0 + row] - a.tbase + lo] = v;
          } else if (pairs_beats(v, (int)col, weak_v[rloc], weak_i[rloc])) {
            // a winner over the row's weakest target: most candidates of a decent model never get here
            const bool excluded = a.mask && ((a.mask[(size_t)row * a.W + (col >> 5)] >> (col & 31)) & 1u);
            if (!excluded)
              for (int t = 0; t < nt; t++)
                if (trow[t] != (int)col && pairs_beats(v, (int)col, tv[rloc * TMAX + t], trow[t])) atomicAdd(&cnt[rloc * TMAX + t], 1);
          }
        }
    }
  }
  if constexpr (COUNT) {
    __syncthreads();
    for (int e = threadIdx.x; e < NL; e += PAIRS_WG) {
      const int r = e / TMAX, t = e - r * TMAX;
      if (t < tn[r] && cnt[e] != 0) atomicAdd(&a.trank[a.tptr[a.u0 + q0 + r] - a.tbase + t], cnt[e]);
    }
  }
}

}  // namespace mfm
