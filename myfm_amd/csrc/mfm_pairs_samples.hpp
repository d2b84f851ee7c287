// mfm_pairs_samples.hpp -- the per-sample selecting form of the query x candidate scorer and the vote over its lists (DESIGN
// 4.13.3): the top k of every query under ONE kept sample at a time -- every sample's own list, the list of the sample drawn for
// a query (Thompson sampling), and the share of the samples whose list holds a candidate (the top-k inclusion probability).
//
// Only the plan, the accumulator and the vote are this file's. The unit of work is a plan entry, (one sample, one row tile of P):
// the workgroup takes a one-sample view of the call's arguments -- Q, the biases, w0 and the cutpoints re-based on sample s, one
// pass of KS / 4 k-steps -- and runs the pieces of mfm_pairs.hpp on it (pairs_contract, pairs_finish_sample, pairs_sample_value,
// pairs_step, PairsSel through pairs_select_stripe), so the value of a pair under sample s is bit for bit the value the moments
// form folds into its mean, and the order is the selection's. The stripes' lists are merged by k_pairs_merge.
//
// Two plans. All samples: P is embedded for every sample as for the other forms, an entry per (sample, row tile of the query
// chunk). Row -> sample: the chunk's rows are grouped by their sample (a stable sort on the host) and k_pairs_embed<., true> writes
// row u's P and bias under sample row_sample[u] alone, in group order, every group padded to whole tiles; an entry per row tile
// of a non-empty group, and row_of gives the chunk's row of a row of P (for the exclusion mask and the way back).
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

// the most list entries of one query row the vote sorts in LDS (a power of two: the sort is bitonic): S * k of a call
constexpr int PAIRS_VOTE_MAX = 32768;
constexpr int PAIRS_VOTE_MAX_TOP = 256;

struct PairsPlanEntry {
  int64_t row0;  // first row of the tile in P's fragment order, a multiple of the form's rows
  int64_t out;   // first list row of the tile within its launch
  int32_t s;     // the sample
  int32_t rows;  // valid rows of the tile
};

// The accumulator of the per-sample form (the interface: PairsMean): the one pass of the one-sample view finishes the value.
template <int MT, int NT, int MODE>
struct PairsOne {
  static constexpr bool PER_SAMPLE = true;
  typedef double Value;
  pairs_d4 v[MT][NT];

  __device__ __forceinline__ void zero() {}
  __device__ __forceinline__ void add(const PairsArgs &a, int s, int64_t q0, int64_t ct0, int lane, const pairs_d4 (&acc)[MT][NT]) {
    const double *__restrict__ cs = MODE == 2 ? a.cut + (size_t)s * a.n_cut : nullptr;
    pairs_finish_sample<MT, NT>(a, s, q0, ct0, lane, acc,
                                [&](int m, int n, int g, double t) { v[m][n][g] = pairs_sample_value<MODE>(t, cs, a.n_cut); });
  }
  __device__ __forceinline__ void rows(const PairsArgs &, int64_t, int) {}
  __device__ __forceinline__ void column(const PairsArgs &, int64_t) {}
  __device__ __forceinline__ double value(const PairsArgs &, int m, int n, int g) const { return v[m][n][g]; }
  static __device__ __forceinline__ double ranked(double v) { return v; }
};

// grid: (the launch's plan entries, stripes)
template <int MT, int NT, int MODE>
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_tile_samples(PairsArgs a) {
  const PairsPlanEntry e = a.plan[blockIdx.x];
  const bool own = a.row_of != nullptr;  // the row -> sample plan: P and its bias hold the row's own sample only
  const size_t ko = (size_t)e.s * a.KS4 * 64;
  PairsArgs b = a;  // the view of sample e.s: sample 0 of 1
  b.Pf = own ? a.Pf : a.Pf + ko;
  b.Qf = a.Qf + ko;
  b.NK = a.KS4;
  b.S = 1;
  b.Ab = own ? a.Ab : a.Ab + (size_t)e.s * a.Upad;
  b.Bb = a.Bb + (size_t)e.s * a.Ipad;
  b.w0s = a.w0s + e.s;
  b.cut = MODE == 2 ? a.cut + (size_t)e.s * a.n_cut : nullptr;
  b.Uc = e.row0 + e.rows;  // (the rows of the tile past it are padding)
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  const int32_t *__restrict__ row_of = a.row_of;
  pairs_select_stripe<MT, NT, PairsOne<MT, NT, MODE>>(b, e.row0, e.out, cb, ce,
                                                      [&](int64_t row) { return own ? (int64_t)row_of[row] : row; });
}

// the merged lists of a launch's entries -> the votes of their query rows: votes[(row * S + s) * k + j], one workgroup per entry
// (all-samples plan: a row of P is the chunk's query row)
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_votes_put(const PairsPlanEntry *__restrict__ plan, const int32_t *__restrict__ out_i, int k,
                                                              int S, int32_t *__restrict__ votes) {
  const PairsPlanEntry e = plan[blockIdx.x];
  for (int t = threadIdx.x; t < e.rows * k; t += PAIRS_WG) {
    const int r = t / k, j = t - r * k;
    votes[((size_t)(e.row0 + r) * S + e.s) * k + j] = out_i[(size_t)(e.out + r) * k + j];
  }
}

// ---- the vote ------------------------------------------------------------------------------------------------------------
// One workgroup per query row over its n = S * k list indices (tails, -1, are no votes): sorts them ascending in LDS (bitonic
// over N >= n, a power of two, padded with INT_MAX), so that a candidate's votes are one run and the runs stand in index order.
// A run that starts at e has at least c votes iff key[e + c - 1] == key[e]: the count threshold -- the largest c that at least
// n_top runs reach, 1 where there are fewer runs -- is found by bisection over c, each probe one counting pass. Kept: every run
// above the threshold and, of the runs exactly at it, the first ones in index order until n_top are kept (a prefix sum over the
// workgroup's contiguous shares gives a run its place among them). The kept entries are then ranked by (count descending, index
// ascending) against each other and written at their rank: index, probability = count / S in fp64; the rest is (-1, 0.0). No
// atomics on the result, nothing depends on the grid.
// dynamic LDS: N ints.
__global__ __launch_bounds__(PAIRS_WG) void k_pairs_vote(const int32_t *__restrict__ votes, int n, int N, int S, int n_top,
                                                         int32_t *__restrict__ out_i, double *__restrict__ out_p) {
  extern __shared__ int vote_key[];
  __shared__ int part[PAIRS_WG];
  __shared__ int sel_i[PAIRS_VOTE_MAX_TOP], sel_c[PAIRS_VOTE_MAX_TOP];
  __shared__ int total, n_sel;
  constexpr int NONE = 2147483647;
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int32_t *__restrict__ mine = votes + (size_t)u * n;
  for (int e = tid; e < N; e += PAIRS_WG) {
    const int c = e < n ? mine[e] : -1;
    vote_key[e] = c < 0 ? NONE : c;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= N; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (N >> 1); t += PAIRS_WG) {
        const int i = 2 * t - (t & (j - 1)), l = i + j;
        const int x = vote_key[i], y = vote_key[l];
        if ((x > y) == ((i & k2) == 0)) {
          vote_key[i] = y;
          vote_key[l] = x;
        }
      }
      __syncthreads();
    }
  // the workgroup's count of the run starts with at least c votes (c >= 1), to every thread
  const auto is_start = [&](int e) { return vote_key[e] != NONE && (e == 0 || vote_key[e - 1] != vote_key[e]); };
  const auto reaches = [&](int e, int c) { return e + c - 1 < N && vote_key[e + c - 1] == vote_key[e]; };
  const auto count_reaching = [&](int c) {
    int mine_n = 0;
    for (int e = tid; e < N; e += PAIRS_WG) mine_n += is_start(e) && reaches(e, c) ? 1 : 0;
    if (tid == 0) total = 0;
    __syncthreads();
    if (mine_n) atomicAdd(&total, mine_n);
    __syncthreads();
    const int t = total;
    __syncthreads();
    return t;
  };
  int thr = 1;
  if (count_reaching(1) > n_top) {
    // the largest c in [1, S] with count_reaching(c) >= n_top (count_reaching falls with c, and count_reaching(1) >= n_top)
    int lo = 1, hi = S;
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (count_reaching(mid) >= n_top)
        lo = mid;
      else
        hi = mid - 1;
    }
    thr = lo;
  }
  const int above = count_reaching(thr + 1);  // all of them are kept; above < n_top unless thr was not raised
  // the runs exactly at the threshold, in index order: a contiguous share of the positions per thread, then a prefix sum
  const int share = (N + PAIRS_WG - 1) / PAIRS_WG;
  const int eb = tid * share < N ? tid * share : N, ee = eb + share < N ? eb + share : N;
  int at_thr = 0;
  for (int e = eb; e < ee; e++) at_thr += is_start(e) && reaches(e, thr) && !reaches(e, thr + 1) ? 1 : 0;
  part[tid] = at_thr;
  if (tid == 0) n_sel = 0;
  __syncthreads();
  int before = 0;
  for (int t = 0; t < tid; t++) before += part[t];
  const int room = n_top - above;  // of the runs at the threshold, the first `room` are kept
  for (int e = eb; e < ee; e++) {
    if (!is_start(e) || !reaches(e, thr)) continue;
    const bool over = reaches(e, thr + 1);
    if (!over && before++ >= room) continue;
    int c = thr;
    if (over) {  // the run's end: the first position past e + thr that holds another key
      int lo = e + thr, hi = N;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (vote_key[mid] == vote_key[e])
          lo = mid + 1;
        else
          hi = mid;
      }
      c = lo - e;
    }
    const int slot = atomicAdd(&n_sel, 1);
    if (slot < PAIRS_VOTE_MAX_TOP) {
      sel_i[slot] = vote_key[e];
      sel_c[slot] = c;
    }
  }
  __syncthreads();
  const int m = n_sel < n_top ? n_sel : n_top;
  for (int j = tid; j < n_top; j += PAIRS_WG) {
    out_i[u * n_top + j] = -1;
    out_p[u * n_top + j] = 0.0;
  }
  __syncthreads();
  for (int t = tid; t < m; t += PAIRS_WG) {
    int rank = 0;
    for (int j = 0; j < m; j++) rank += sel_c[j] > sel_c[t] || (sel_c[j] == sel_c[t] && sel_i[j] < sel_i[t]) ? 1 : 0;
    out_i[u * n_top + rank] = sel_i[t];
    out_p[u * n_top + rank] = (double)sel_c[t] / (double)S;
  }
}

}  // namespace mfm
