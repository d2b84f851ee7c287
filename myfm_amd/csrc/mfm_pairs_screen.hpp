// mfm_pairs_screen.hpp -- the screened top-k (mfm_pairs_topk_screened*): the list of mfm_pairs_topk, bit for bit, for the
// rows whose list a bf16 contraction can certify, at a fraction of the fp64 contraction's cost. Mode 0 only: the value is linear in
//   r(u, i) = Bsum[i] + sum_e P[u, e] Q[i, e],   S v(u, i) = c_u + r(u, i),   c_u = w0sum + Asum[u],   e over the L = S KS inner elements.
//   k_screen_pack     P or Q (fp64, fragment order of the f64 MFMA) -> bf16 in the fragment order of v_mfma_f32_16x16x32_bf16, the
//                     rows' 2-norms and a flag per row whose operands leave the range the bound is derived for
//   k_screen_tile     r~ = Bsum[i] + (double)(bf16 contraction, fp32 accumulators); the k_s best per row through PairsSel, or dense
//   k_screen_rescore  the exact value of every shortlisted pair: pairs_contract's own chain of f64 MFMAs and PairsMean<., ., 0>'s finish
//   k_screen_finish   the shortlist in the exact order, its first k, and the certificate that nothing left out can belong to them
// Error model (u = 2^-8, the unit roundoff of bf16 under round to nearest even): |r~ - r| <= e_u = eps |P_u| max_i |Q_i| with
//   eps = (2 u + u^2) + gamma (1 + u)^2,   gamma = n c 2^-24 / (1 - n c 2^-24),   n the padded inner length,
// the first term from rounding the operands (a bf16 x bf16 product is exact in fp32; Cauchy-Schwarz), the second the fp32 accumulation
// with the constant c = SCREEN_C_ACC, which is measured, not derived. Operands of magnitude in [2^-50, 2^50] or zero
// keep every product and every rounded operand a normal fp32 number, so the relative model holds; a row or candidate outside is
// flagged and not certified, and an accumulator that is not finite counts as +inf (shortlisted, never a reason to leave a pair out).
#pragma once
#include "mfm_pairs.hpp"

namespace mfm {

constexpr int SCREEN_MAX_K = 128;      // the k of a screened call; the shortlist has k_s = min(256, max(64, 2 k)) entries
constexpr int SCREEN_INNER = 32;       // inner elements of one bf16 MFMA
constexpr int SCREEN_COL_ALIGN = 1024; // the bf16 candidates are padded to the widest workgroup step (MT = 1: 4 waves x 16 tiles)
constexpr double SCREEN_U = 0x1p-8;    // bf16: 8 significand bits
constexpr double SCREEN_C_ACC = 4.0;   // fp32 accumulation: roundings per inner element assumed of the matrix unit (measured: 4.0e-3)

typedef uint32_t screen_u4 __attribute__((ext_vector_type(4)));
typedef __bf16 screen_bf8 __attribute__((ext_vector_type(8)));
typedef float screen_f4 __attribute__((ext_vector_type(4)));

// eps of the error model for a padded inner length n; +inf where the model gives nothing (n c 2^-24 >= 1/2)
inline double screen_eps(int64_t n) {
  const double g = (double)n * SCREEN_C_ACC * 0x1p-24;
  if (g >= 0.5) return INFINITY;
  const double u = SCREEN_U;
  return (2.0 * u + u * u) + g / (1.0 - g) * (1.0 + u) * (1.0 + u);
}

// what the certificate needs next to the lists (device arrays; Asum and w0sum as in PairsArgs)
struct ScreenBound {
  const double *pnorm;        // [Upad]: |P_u|_2 over L
  const int32_t *pflag;       // [Upad]: the row is outside the model's range
  const int32_t *cand_flag;   // [1]: some candidate is
  const double *cmax;         // [2]: max_i |Q_i|_2, max_i |Bsum_i|
  const double *Asum;
  double w0sum, eps, L;
  int S;
  // e_u / S and delta_u of row u: the bf16 path's error and the fp64 roundings of either path, in units of the value
  __device__ __forceinline__ void terms(int64_t u, double &c_u, double &e_over_s, double &delta) const {
    c_u = w0sum + Asum[u];
    const double pq = pnorm[u] * cmax[0];
    e_over_s = eps * pq / (double)S;
    delta = (L + 8.0) * 0x1p-53 * (fabs(c_u) + cmax[1] + pq) / (double)S;
  }
};

// ---- pack ------------------------------------------------------------------------------------------------------------------------
// double -> bf16 bits, round to nearest even in ONE rounding (through float it would be two). Below the normal range: zero.
__device__ __forceinline__ uint32_t screen_bf16(double x) {
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  const uint32_t sign = (uint32_t)(b >> 48) & 0x8000u;
  const uint64_t m = b & 0x7fffffffffffffffull;
  if (m > 0x7ff0000000000000ull) return sign | 0x7fc0u;                            // NaN
  const uint64_t r = (m + ((1ull << 44) - 1) + ((m >> 45) & 1ull)) >> 45;          // (exponent, 7 bits): a carry moves the exponent
  const int e8 = (int)(r >> 7) - 1023 + 127;
  if (e8 <= 0) return sign;
  if (e8 >= 255) return sign | 0x7f80u;
  return sign | ((uint32_t)e8 << 7) | ((uint32_t)r & 0x7fu);
}

// an operand the error model does not cover: not finite, or not zero and outside [2^-50, 2^50]
__device__ __forceinline__ int screen_bad(double x) {
  const double m = fabs(x);
  return !(m == 0.0 || (m >= 0x1p-50 && m <= 0x1p50)) ? 1 : 0;
}

// One workgroup per 16-row tile t of a side. Wave w converts the inner chunks w, w + 4, ...: lane l takes the 8 inner elements from
// 32 c + 8 (l >> 4) of row l & 15 and writes them as its 16 bytes of (tile, chunk) -- the operand of v_mfma_f32_16x16x32_bf16 for
// that lane, so a wave's fragment load is 1 KB contiguous. Elements at or beyond L and tiles at or beyond src_tiles (the padding up
// to SCREEN_COL_ALIGN, which Xf does not have) are zeros. Then the rows' sums of squares, partials added in (wave, lane >> 4) order.
__global__ __launch_bounds__(PAIRS_WG) void k_screen_pack(const double *__restrict__ Xf, int64_t NK, int64_t src_tiles, int NC,
                                                          const double *__restrict__ bias_sum, screen_u4 *__restrict__ Xb,
                                                          double *__restrict__ norm, int32_t *__restrict__ flag,
                                                          int32_t *__restrict__ any_flag) {
  __shared__ double s_sq[PAIRS_WG];
  __shared__ int s_bad[PAIRS_WG];
  const int64_t t = blockIdx.x, L = NK * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool src = t < src_tiles;
  double sq = 0.0;
  int bad = 0;
  for (int c = wave; c < NC; c += PAIRS_WG / 64) {
    uint32_t h[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int64_t e = (int64_t)c * SCREEN_INNER + 8 * (lane >> 4) + j;
      const double x = src && e < L ? Xf[((size_t)t * NK + (e >> 2)) * 64 + (e & 3) * 16 + (lane & 15)] : 0.0;
      sq += x * x;
      bad |= screen_bad(x);
      h[j] = screen_bf16(x);
    }
    Xb[((size_t)t * NC + c) * 64 + lane] = (screen_u4){h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
  }
  s_sq[threadIdx.x] = sq;
  s_bad[threadIdx.x] = bad;
  __syncthreads();
  if (threadIdx.x < 16) {
    sq = 0.0;
    bad = 0;
    for (int p = 0; p < PAIRS_WG / 16; p++) {
      sq += s_sq[p * 16 + threadIdx.x];
      bad |= s_bad[p * 16 + threadIdx.x];
    }
    const int64_t r = t * 16 + threadIdx.x;
    if (src && bias_sum && !isfinite(bias_sum[r])) bad = 1;
    norm[r] = sqrt(sq);
    flag[r] = bad;
    if (bad && any_flag) atomicOr(any_flag, 1);
  }
}

// max_i |Q_i| and max_i |Bsum_i| over the candidates, one workgroup
__global__ __launch_bounds__(PAIRS_WG) void k_screen_cand_max(const double *__restrict__ qnorm, const double *__restrict__ Bsum, int64_t I,
                                                              double *__restrict__ out) {
  __shared__ double s_q[PAIRS_WG], s_b[PAIRS_WG];
  double mq = 0.0, mb = 0.0;
  for (int64_t i = threadIdx.x; i < I; i += PAIRS_WG) {
    mq = fmax(mq, qnorm[i]);
    mb = fmax(mb, fabs(Bsum[i]));
  }
  s_q[threadIdx.x] = mq;
  s_b[threadIdx.x] = mb;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int p = 1; p < PAIRS_WG; p++) {
      mq = fmax(mq, s_q[p]);
      mb = fmax(mb, s_b[p]);
    }
    out[0] = mq;
    out[1] = mb;
  }
}

// ---- screen ----------------------------------------------------------------------------------------------------------------------
struct ScreenArgs {
  PairsArgs a;                 // the selection's share: Bsum, mask, W, k = k_s, the stripes' lists, Uc, I, stripe_len, dense
  const screen_u4 *Pb, *Qb;    // bf16 operands: [rows / 16][NC][64 lanes] x 16 bytes
  int NC;                      // inner chunks of 32
};

template <int MT>
constexpr size_t screen_stage_bytes() { return (size_t)2 * MT * 64 * sizeof(screen_u4); }

// A workgroup owns MT * 16 query rows and one stripe of candidates, walked in steps of 4 * NT * 16, NT = 16 / MT: wave w holds the
// MT x NT accumulator tiles (64 fp32 registers) at candidate tiles [ct0, ct0 + NT), ct0 = step / 16 + w NT. Per inner chunk the
// query operand -- shared by the four waves -- is staged once in LDS, in two buffers: the next chunk's 16 bytes per thread are
// loaded from global memory before this chunk's MFMAs issue and stored to the other buffer after them, one barrier per chunk. A
// candidate fragment is used by one wave only: global memory -> registers, one chunk ahead. f32 C/D map: lane l, register g hold
// (row 4 (l >> 4) + g, column l & 15). The selection's LDS (PairsSel<MT>) comes first, the stages behind it.
template <int MT, bool DENSE>
__global__ __launch_bounds__(PAIRS_WG) void k_screen_tile(ScreenArgs sa) {
  constexpr int NT = 16 / MT, STEP = 4 * NT * 16, STAGE = MT * 64;
  extern __shared__ double pairs_smem[];
  const PairsArgs &a = sa.a;
  screen_u4 *stage = (screen_u4 *)((char *)pairs_smem + (DENSE ? 0 : PairsSel<MT>::BYTES));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NC = sa.NC;
  const int64_t q0 = (int64_t)blockIdx.x * (MT * 16);
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  PairsSel<MT> sel;
  if constexpr (!DENSE) sel.init(a.k);
  const bool stager = tid < STAGE;
  const screen_u4 *pa = sa.Pb + ((size_t)((q0 >> 4) + (tid >> 6)) * NC) * 64 + lane;  // (read by stagers only)
  for (int64_t c0 = cb; c0 < ce; c0 += STEP) {
    const int64_t ct0 = (c0 >> 4) + wave * NT;
    const screen_u4 *pq = sa.Qb + (size_t)ct0 * NC * 64 + lane;
    screen_f4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int n = 0; n < NT; n++) acc[m][n] = (screen_f4){0.f, 0.f, 0.f, 0.f};
    screen_u4 bn[NT], an = (screen_u4){0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < NT; n++) bn[n] = (screen_u4){0, 0, 0, 0};
    if (NC > 0) {
      if (stager) stage[tid] = pa[0];
#pragma unroll
      for (int n = 0; n < NT; n++) bn[n] = pq[(size_t)n * NC * 64];
    }
    __syncthreads();
    for (int c = 0; c < NC; c++) {
      screen_u4 bc[NT], ac[MT];
#pragma unroll
      for (int n = 0; n < NT; n++) bc[n] = bn[n];
      const bool more = c + 1 < NC;
      if (more) {
        if (stager) an = pa[(size_t)(c + 1) * 64];
#pragma unroll
        for (int n = 0; n < NT; n++) bn[n] = pq[((size_t)n * NC + c + 1) * 64];
      }
      const screen_u4 *cur = stage + (c & 1) * STAGE;
#pragma unroll
      for (int m = 0; m < MT; m++) ac[m] = cur[m * 64 + lane];
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int n = 0; n < NT; n++)
          acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(screen_bf8, ac[m]), __builtin_bit_cast(screen_bf8, bc[n]),
                                                              acc[m][n], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // (the chunk's MFMAs issue before the wait for the next chunk's operands, as in pairs_contract)
      if (more && stager) stage[((c + 1) & 1) * STAGE + tid] = an;
      __syncthreads();
    }
    // r~ = Bsum[i] + (double)acc, tile column by tile column: a round of the selection is one tile column per wave
#pragma unroll
    for (int n = 0; n < NT; n++) {
      const int64_t col = (ct0 + n) * 16 + (lane & 15);
      const bool col_ok = col < ce;
      const double bs = col_ok ? a.Bsum[col] : 0.0;
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
          const int rloc = m * 16 + 4 * (lane >> 4) + g;
          const int64_t row = q0 + rloc;
          const float f = acc[m][n][g];
          const double r = isfinite(f) ? bs + (double)f : (double)INFINITY;
          if (!col_ok || row >= a.Uc) continue;
          if constexpr (DENSE)
            a.dense[(size_t)row * a.I + col] = r;
          else
            sel.push(a, rloc, row, col, r);
        }
      if constexpr (!DENSE) sel.round();
    }
  }
  if constexpr (!DENSE) sel.finish(a, q0);
}

// ---- rescore ---------------------------------------------------------------------------------------------------------------------
// One wave per (query row u, group of 16 of the n_short first entries of its merged list sl_i[u][ks], (ks + 15) / 16 groups; an empty
// entry gives -inf, ex_v is written for e < n_short only).
// A: the row's own 16-row tile of P, the usual 512-byte load. B: gathered, lane l reads inner step l >> 4 of candidate idx[l & 15]
// from the fragment-ordered Q. Then pairs_contract's mode-0 chain: every k-step in order into one accumulator from zero -- an MFMA
// output element depends on its own row and column operands alone, so the element (u & 15, j) is bit for bit the tile kernel's for
// that pair -- and PairsMean<., ., 0>'s finish. Lanes with l >> 4 == u & 3 hold row u & 15 in register (u & 15) >> 2.
__global__ __launch_bounds__(PAIRS_WG) void k_screen_rescore(PairsArgs a, const int32_t *__restrict__ sl_i, int ks, int n_short,
                                                             double *__restrict__ ex_v) {
  const int lane = threadIdx.x & 63, G = (ks + 15) >> 4;
  const int64_t w = (int64_t)blockIdx.x * (PAIRS_WG / 64) + (threadIdx.x >> 6);
  const int64_t u = w / G;
  if (u >= a.Uc) return;
  const int e = (int)(w - u * G) * 16 + (lane & 15);
  const int ci = e < n_short ? sl_i[(size_t)u * ks + e] : -1;
  const int64_t c = ci < 0 ? 0 : ci;
  const double *pa = a.Pf + (size_t)(u >> 4) * a.p_stride * 64 + lane;
  const double *pq = a.Qf + (size_t)(c >> 4) * a.q_stride * 64 + (lane >> 4) * 16 + (c & 15);
  pairs_d4 acc = (pairs_d4){0.0, 0.0, 0.0, 0.0};
  for (int64_t q = 0; q < a.NK; q++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[q * 64], pq[q * 64], acc, 0, 0, 0);
  const int g = (int)(u & 15) >> 2;
  const double tot = g == 0 ? acc[0] : g == 1 ? acc[1] : g == 2 ? acc[2] : acc[3];
  if ((lane >> 4) != (int)(u & 3) || e >= n_short) return;  // (the last group may reach beyond the shortlist: nothing is written there)
  const double asum = a.w0sum + a.Asum[u], bsum = a.Bsum[c], div = (double)a.S;
  ex_v[(size_t)u * ks + e] = ci < 0 ? -INFINITY : ((asum + bsum) + tot) / div;
}

// ---- finish ----------------------------------------------------------------------------------------------------------------------
// One wave per query row: the shortlist (the first ks - 1 entries of the merged list, with their exact values) ranked by counting
// under the selection's total order, the first k written (tail -1 / -inf), and the certificate. t_u, the approximate value of the
// list's last entry, bounds r~ of every candidate left out, so such a candidate's value is at most (c_u + t_u + e_u) / S + delta_u
// as this kernel computes it:   certified  <=>  v_k > (c_u + t_u + e_u) / S + 2 delta_u,   strictly.
// A list that is not full left nothing out: certified whatever v_k is. Never certified: a flagged row, any flagged candidate, a c_u
// that is not finite (then, and only then, a value may be NaN and the ranks below need not be a permutation).
__global__ __launch_bounds__(PAIRS_WG) void k_screen_finish(const double *__restrict__ sl_v, const int32_t *__restrict__ sl_i,
                                                            const double *__restrict__ ex_v, int ks, int k, int64_t Uc, ScreenBound b,
                                                            double *__restrict__ out_v, int32_t *__restrict__ out_i,
                                                            uint8_t *__restrict__ cert) {
  __shared__ double s_v[PAIRS_WG / 64][PAIRS_MAX_K], s_vk[PAIRS_WG / 64];
  __shared__ int s_i[PAIRS_WG / 64][PAIRS_MAX_K];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_short = ks - 1;
  const int64_t u = (int64_t)blockIdx.x * (PAIRS_WG / 64) + wave;
  const bool live = u < Uc;
  double ev[4];
  int ei[4], rk[4], n_valid = 0;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int e = lane + 64 * t;
    const bool in = live && e < n_short;
    ei[t] = in ? sl_i[(size_t)u * ks + e] : -1;
    ev[t] = in ? ex_v[(size_t)u * ks + e] : -INFINITY;
    rk[t] = 0;
    s_v[wave][e] = ev[t];
    s_i[wave][e] = ei[t];
    n_valid += __popcll(__ballot(ei[t] >= 0));
  }
  if (lane == 0) s_vk[wave] = -INFINITY;
  __syncthreads();
  for (int j = 0; j < n_valid; j++) {  // (the merged list's valid entries are a prefix)
    const double vj = s_v[wave][j];
    const int ij = s_i[wave][j];
#pragma unroll
    for (int t = 0; t < 4; t++) rk[t] += pairs_beats(vj, ij, ev[t], ei[t]) ? 1 : 0;
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (ei[t] >= 0 && rk[t] < k) {
      out_v[(size_t)u * k + rk[t]] = ev[t];
      out_i[(size_t)u * k + rk[t]] = ei[t];
      if (rk[t] == k - 1) s_vk[wave] = ev[t];
    }
  if (live)
    for (int j = n_valid + lane; j < k; j += 64) {
      out_v[(size_t)u * k + j] = -INFINITY;
      out_i[(size_t)u * k + j] = -1;
    }
  __syncthreads();
  if (!live || lane != 0) return;
  double c_u, e_over_s, delta;
  b.terms(u, c_u, e_over_s, delta);
  bool ok = !b.pflag[u] && !*b.cand_flag && isfinite(c_u);
  if (ok && sl_i[(size_t)u * ks + ks - 1] >= 0) {
    const double t_u = sl_v[(size_t)u * ks + ks - 1];
    ok = s_vk[wave] > ((c_u + t_u) / (double)b.S + e_over_s) + 2.0 * delta;
  }
  cert[u] = ok ? 1 : 0;
}

// the dense diagnostic's second output: E_u = e_u / S + delta_u per row, so that |r~ - r| <= S E_u
__global__ __launch_bounds__(PAIRS_WG) void k_screen_bound(ScreenBound b, int64_t Uc, double *__restrict__ E) {
  const int64_t u = (int64_t)blockIdx.x * PAIRS_WG + threadIdx.x;
  if (u >= Uc) return;
  double c_u, e_over_s, delta;
  b.terms(u, c_u, e_over_s, delta);
  E[u] = e_over_s + delta;
}

}  // namespace mfm
