// mfm_pairs_rank.hpp -- ranks of given (query, candidate) pairs among all candidates of their query. The rank of
// a target pair is the number of admissible candidates (valid, not excluded, not the target itself) that beat it under the total
// order of the selection, pairs_beats: value descending, candidate index ascending. It is an exact integer count, independent of
// tiles, stripes and chunks. The embeddings, the exclusion mask and the stripes are those of mfm_pairs.hpp.
//
// Two passes of one kernel over the same fragment-ordered P and Q. Both finish their values with pairs_step over PairsMean, the
// very code of the dense and the selecting mean forms (mfm_pairs.hpp), so a value finished here is bit for bit the one those
// forms finish for that pair. What is this file's: the targets in LDS, the walk over the steps, and what becomes of a value:
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
constexpr int PAIRS_RANK_ROWS = 64;   // query rows of a workgroup: the target lists are laid out for MT = 4

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
  typedef PairsMean<MT, NT, MODE> Acc;
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
  if constexpr (!COUNT) {
    // ---- the values at the targets. Every barrier of this loop is reached by all threads: nx is the workgroup's.
    int cur = 0;  // threads [0, ROWS): the first target of the thread's row at or after the step under way
    for (int64_t c0 = cb; c0 < ce; c0 += CT) {
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
      pairs_step<MT, NT, Acc>(
          a, q0, c0, ce,
          [&](int rloc, int64_t row, int64_t col, double v) {
            // the column's place in the row's sorted target list, if it has one
            const int nt = tn[rloc];
            const int *__restrict__ trow = ti + rloc * TMAX;
            int lo = 0, hi = nt;
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (trow[mid] < (int)col)
                lo = mid + 1;
              else
                hi = mid;
            }
            if (lo < nt && trow[lo] == (int)col) a.tval[a.tptr[a.u0 + row] - a.tbase + lo] = v;
          },
          [] {});
    }
  } else {
    // ---- the counts, over every step of the stripe
    for (int64_t c0 = cb; c0 < ce; c0 += CT)
      pairs_step<MT, NT, Acc>(
          a, q0, c0, ce,
          [&](int rloc, int64_t row, int64_t col, double v) {
            // a winner over the row's weakest target: most candidates of a decent model never get here
            if (!pairs_beats(v, (int)col, weak_v[rloc], weak_i[rloc])) return;
            const bool excluded = a.mask && ((a.mask[(size_t)row * a.W + (col >> 5)] >> (col & 31)) & 1u);
            if (excluded) return;
            const int nt = tn[rloc];
            const int *__restrict__ trow = ti + rloc * TMAX;
            for (int t = 0; t < nt; t++)
              if (trow[t] != (int)col && pairs_beats(v, (int)col, tv[rloc * TMAX + t], trow[t])) atomicAdd(&cnt[rloc * TMAX + t], 1);
          },
          [] {});
    __syncthreads();
    for (int e = threadIdx.x; e < NL; e += PAIRS_WG) {
      const int r = e / TMAX, t = e - r * TMAX;
      if (t < tn[r] && cnt[e] != 0) atomicAdd(&a.trank[a.tptr[a.u0 + q0 + r] - a.tbase + t], cnt[e]);
    }
  }
}

}  // namespace mfm
