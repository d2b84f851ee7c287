// mfm_pairs_diverse.hpp -- the diversified top-k of the query x candidate family: greedy maximal marginal relevance
// (Carbonell & Goldstein 1998) over a pool of M <= 128 candidates per query row. The pool is mfm_pairs_topk's list of length M,
// produced by that form's own launch and left on the device. With v_0 >= ... the pool's values, n_live its entries with index >= 0,
//   rel_j    = (v_j - v_min) / (v_0 - v_min), v_min the last live value; 1 where v_0 == v_min,
//   sim(i,j) = (1 / S) sum_s c_s(i, j), c_s the per-sample cosine of mfm_pairs_sim.hpp between candidate rows i and j,
//   step 0 takes pool position 0; step t >= 1 the unchosen live position j of largest g_t(j) = lam rel_j - (1 - lam) max_c sim(j, c)
//   over the positions c chosen so far, ties to the lower position.
//
// Two kernels.
//   k_div_pack    once per call: the candidate side's resident fragment-ordered Q -> Qh[I][Lpad] row-major, every sample's factors
//                 multiplied by that sample's r = 1 / sqrt(sum_k Q_k^2) (0 where the sum is 0, the squares summed in factor order as
//                 k_pairs_embed<., ., 1> sums them), the inner length L = S KS padded with zeros to a multiple of 8. S sim(i, j) is
//                 then ONE inner product of length L, and a gathered row is one contiguous stream (a row gathered out of the fragment
//                 order touches a 128-byte line for 8 useful bytes).
//   k_div_select  one workgroup of 4 waves per query row: the Gram matrix of the gathered pool rows on v_mfma_f64_16x16x4_f64 into
//                 LDS, then the greedy steps on wave 0 alone.
// Neither kernel holds a float: no packed fp32 instruction can be selected for them.
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

constexpr int DIV_MAX_POOL = 128;
constexpr int DIV_CH = 2;         // MFMA steps per staged chunk: one 16-byte run per (row, quarter)
constexpr int DIV_WAVE_TILES = 9; // upper-triangle 16 x 16 tiles per wave at 8 tile rows: 36 / 4

typedef double div_d2 __attribute__((ext_vector_type(2)));

// the padded inner length of Qh, and the dynamic LDS of k_div_select for pools of up to Mp = 16 ceil(M / 16) rows: the Gram matrix
// [Mp][Mp] and two stages [Mp][4][DIV_CH], all fp64 (144 KB at Mp = 128, of gfx950's 160 KB)
constexpr int64_t div_padded_length(int64_t L) { return (L + 4 * DIV_CH - 1) / (4 * DIV_CH) * (4 * DIV_CH); }
constexpr size_t div_lds_bytes(int Mp) { return ((size_t)Mp * Mp + 2 * (size_t)Mp * 4 * DIV_CH) * sizeof(double); }

// One thread per (candidate row i, sample s). Q's fragment order (k_pairs_embed): value (row r, k-step q = s KS4 + k / 4, factor k & 3)
// at ((r >> 4) NK + q) 64 + (k & 3) 16 + (r & 15). The thread of the last sample writes the row's zero padding [L, Lpad).
__global__ __launch_bounds__(PAIRS_WG) void k_div_pack(const double *__restrict__ Qf, int64_t NK, int KS4, int S, int64_t I, int64_t Lpad,
                                                       double *__restrict__ Qh) {
  const int64_t i = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (i >= I) return;
  const int s = blockIdx.y;
  const double *__restrict__ src = Qf + ((i >> 4) * NK + (int64_t)s * KS4) * 64 + (i & 15);
  double sq = 0.0;
  for (int q = 0; q < KS4; q++)
#pragma unroll
    for (int f = 0; f < 4; f++) {
      const double v = src[(int64_t)q * 64 + f * 16];
      sq += v * v;
    }
  const double r = sq > 0.0 ? 1.0 / sqrt(sq) : 0.0;
  double *__restrict__ row = Qh + i * Lpad;
  pairs_d4 *__restrict__ dst = (pairs_d4 *)(row + (int64_t)s * KS4 * 4);  // (32-byte aligned: Lpad is a multiple of 8, KS of 4)
  for (int q = 0; q < KS4; q++) {
    const double *__restrict__ p = src + (int64_t)q * 64;
    dst[q] = (pairs_d4){p[0] * r, p[16] * r, p[32] * r, p[48] * r};
  }
  if (s == S - 1)
    for (int64_t e = (int64_t)S * KS4 * 4; e < Lpad; e++) row[e] = 0.0;
}

struct DivArgs {
  const double *Qh = nullptr;        // [I][Lpad], k_div_pack's
  int64_t Lpad = 0;
  const double *pool_v = nullptr;    // [rows][M]: the merged top-M lists of the chunk's rows, in the selection's total order
  const int32_t *pool_i = nullptr;   // (tail: index -1)
  int M = 0, k = 0, S = 1;
  double lam = 0.0;
  int32_t *out_i = nullptr;          // [rows][k]
  double *out_v = nullptr, *out_g = nullptr, *out_r = nullptr;
};
static_assert(std::is_trivially_copyable<DivArgs>::value, "DivArgs is a kernel argument");

// The Gram matrix. With NT = ceil(n_live / 16) tile rows the NT (NT + 1) / 2 upper-triangle tiles are dealt to the waves round robin
// (tile n to wave n & 3, at most DIV_WAVE_TILES each, 4 accumulator registers per tile). The inner dimension is walked in chunks of
// DIV_CH MFMA steps staged through two LDS buffers: thread `it` (and it + 256) owns (pool row it >> 2, quarter it & 3) and loads that
// row's next 16 bytes of its quarter's run -- element quarter * Lpad / 4 + DIV_CH chunk + step -- before the current chunk's MFMAs,
// stores them into the other buffer after, one barrier per chunk. A Gram matrix contracts the same staged rows on both sides, so the
// inner index may be permuted as long as both operands take the same permutation: lane (row l & 15, quarter l >> 4) of either operand
// takes MFMA step s of a chunk from its quarter's run, and a lane's operand load is the 16 bytes its loader thread stored. Rows of
// padding and pool entries >= n_live are staged as zeros. The finished tiles are divided by S and written to G[Mp][Mp] in LDS, tile
// (a, b) with a < b mirrored, so the greedy steps read row c of G contiguously.
// The greedy steps run on wave 0 over LDS: lane l holds pool positions l and l + 64 (rel, the running max-sim, unchosen or not, in
// registers), the arg-max is a wave reduction on (g descending, position ascending) -- a NaN g compares as -inf --, and the lane that
// owns the chosen position writes the step's outputs. No workgroup barrier inside the loop: waves 1 to 3 have left.
__global__ __launch_bounds__(PAIRS_WG) void k_div_select(DivArgs a) {
  extern __shared__ double div_smem[];
  __shared__ double s_val[DIV_MAX_POOL];
  __shared__ int s_idx[DIV_MAX_POOL];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t u = blockIdx.x;
  const size_t o = (size_t)u * a.k;
  if (tid < a.M) {
    s_idx[tid] = a.pool_i[u * a.M + tid];
    s_val[tid] = a.pool_v[u * a.M + tid];
  }
  __syncthreads();
  const int n_live = __popcll(__ballot(lane < a.M && s_idx[lane < a.M ? lane : 0] >= 0)) +
                     __popcll(__ballot(lane + 64 < a.M && s_idx[lane + 64 < a.M ? lane + 64 : 0] >= 0));
  if (n_live == 0) {
    for (int t = tid; t < a.k; t += PAIRS_WG) {
      a.out_i[o + t] = -1;
      a.out_v[o + t] = -INFINITY;
      a.out_g[o + t] = __builtin_nan("");
      a.out_r[o + t] = __builtin_nan("");
    }
    return;
  }
  const int NT = (n_live + 15) >> 4, Mp = NT * 16, ntri = NT * (NT + 1) / 2;
  double *__restrict__ G = div_smem;
  double *__restrict__ stage = G + Mp * Mp;  // [2][Mp][4][DIV_CH]

  // ---- this wave's tiles
  int ta[DIV_WAVE_TILES], tb[DIV_WAVE_TILES];
#pragma unroll
  for (int t = 0; t < DIV_WAVE_TILES; t++) {
    int row = 0, rem = wave + 4 * t;
    while (row < NT && rem >= NT - row) {
      rem -= NT - row;
      row++;
    }
    ta[t] = row;  // (row == NT: past the last tile, never used)
    tb[t] = row + rem;
  }
  const int n_mine = ntri > wave ? (ntri - wave + 3) >> 2 : 0;

  // ---- the loader's two (row, quarter) runs
  const int64_t Lq = a.Lpad >> 2;
  const int nch = (int)(Lq / DIV_CH);
  const double *src[2];
  bool has[2];
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int it = tid + PAIRS_WG * e, row = it >> 2;
    has[e] = it < Mp * 4;
    src[e] = has[e] && row < n_live ? a.Qh + (int64_t)s_idx[row] * a.Lpad + (int64_t)(it & 3) * Lq : nullptr;
  }
  div_d2 nx[2];
  const auto fetch = [&](int ch) {
#pragma unroll
    for (int e = 0; e < 2; e++) nx[e] = src[e] ? *(const div_d2 *)(src[e] + (int64_t)ch * DIV_CH) : (div_d2){0.0, 0.0};
  };
  const auto put = [&](int buf) {
#pragma unroll
    for (int e = 0; e < 2; e++)
      if (has[e]) *(div_d2 *)(stage + buf * Mp * 4 * DIV_CH + (tid + PAIRS_WG * e) * DIV_CH) = nx[e];
  };

  pairs_d4 acc[DIV_WAVE_TILES];
#pragma unroll
  for (int t = 0; t < DIV_WAVE_TILES; t++) acc[t] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
  if (nch > 0) {
    fetch(0);
    put(0);
  }
  __syncthreads();
  const int lane_off = ((lane & 15) * 4 + (lane >> 4)) * DIV_CH;
  for (int ch = 0; ch < nch; ch++) {
    if (ch + 1 < nch) fetch(ch + 1);
    const double *__restrict__ st = stage + (ch & 1) * Mp * 4 * DIV_CH + lane_off;
#pragma unroll
    for (int t = 0; t < DIV_WAVE_TILES; t++)
      if (t < n_mine) {
        const div_d2 A = *(const div_d2 *)(st + ta[t] * 16 * 4 * DIV_CH);
        const div_d2 B = ta[t] == tb[t] ? A : *(const div_d2 *)(st + tb[t] * 16 * 4 * DIV_CH);
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.x, B.x, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(A.y, B.y, acc[t], 0, 0, 0);
      }
    if (ch + 1 < nch) put((ch + 1) & 1);
    __syncthreads();
  }

  // ---- sim = Gram / S into LDS (f64 C/D map: lane l, register g hold (row (l >> 4) + 4 g, column l & 15))
  const double n_s = (double)a.S;
#pragma unroll
  for (int t = 0; t < DIV_WAVE_TILES; t++)
    if (t < n_mine) {
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int row = ta[t] * 16 + (lane >> 4) + 4 * g, col = tb[t] * 16 + (lane & 15);
        const double v = acc[t][g] / n_s;
        G[row * Mp + col] = v;
        if (ta[t] != tb[t]) G[col * Mp + row] = v;
      }
    }
  __syncthreads();
  if (wave != 0) return;

  // ---- the greedy steps
  const double v_min = s_val[n_live - 1], span = s_val[0] - v_min;
  double rel[2], ms[2];
  bool open[2];
#pragma unroll
  for (int e = 0; e < 2; e++) {
    const int j = lane + 64 * e;
    open[e] = j < n_live;
    rel[e] = !open[e] ? 0.0 : span == 0.0 ? 1.0 : (s_val[j] - v_min) / span;
    ms[e] = -INFINITY;
  }
  for (int t = 0; t < a.k; t++) {
    if (t >= n_live) {
      if (lane == 0) {
        a.out_i[o + t] = -1;
        a.out_v[o + t] = -INFINITY;
        a.out_g[o + t] = __builtin_nan("");
        a.out_r[o + t] = __builtin_nan("");
      }
      continue;
    }
    double g[2], bg = -INFINITY;
    int bp = 2147483647;
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int j = lane + 64 * e;
      g[e] = t == 0 ? a.lam * rel[e] : a.lam * rel[e] - (1.0 - a.lam) * ms[e];
      if (!open[e] || (t == 0 && j != 0)) continue;
      const double gc = g[e] == g[e] ? g[e] : -INFINITY;
      if (gc > bg || (gc == bg && j < bp)) {
        bg = gc;
        bp = j;
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double og = __shfl_xor(bg, off);
      const int op = __shfl_xor(bp, off);
      if (og > bg || (og == bg && op < bp)) {
        bg = og;
        bp = op;
      }
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int j = lane + 64 * e;
      if (j == bp) {
        a.out_i[o + t] = s_idx[j];
        a.out_v[o + t] = s_val[j];
        a.out_g[o + t] = g[e];
        a.out_r[o + t] = t == 0 ? 0.0 : ms[e];
        open[e] = false;
      }
      if (open[e]) ms[e] = fmax(ms[e], G[bp * Mp + j]);
    }
  }
}

}  // namespace mfm
