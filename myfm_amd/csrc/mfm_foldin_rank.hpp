// mfm_foldin_rank.hpp -- kernels of mfm_foldin_rank_* (mfm_foldin_rank.hip): every candidate context scored for every
// new entity under the entity's OWN posterior. Under kept sample s the parameters of new entity u are N(theta_us, Lambda_us^-1)
// (mfm_foldin.hpp), so the score of pair (u, c) -- the row X_cand[c] + e_u -- is normal under that sample,
//   m_usc = f_sc + z_sc^T theta_us,   v_usc = z_sc^T Lambda_us^-1 z_sc = |W_us z_sc|^2,   W_us = U_us^-T  (Lambda = U^T U),
// and over the S samples a mixture of S normals:
//   mean = 1/S sum_s m,  std_within^2 = 1/S sum_s v,  std^2 = std_within^2 + 1/S sum_s (m - mean)^2,  gain = 1/S sum_s 1/2 log1p(alpha_s v).
// k_foldin<false, true> keeps [W_us; theta_us^T] as an (M + 1) x M left operand in MFMA fragment order (foldin_keep_*), k_foldin_rank_cand
// writes z_sc of all candidates as the right operand and f_sc, k_foldin_rank_tile contracts: one product gives W z (its squared norm is
// v) and, in row M, m - f. The left operand differs for every (entity, sample), so this is a batched triangular contraction, not the
// pair scorer's (which shares one operand per sample across the queries): the candidates' z of one sample are staged in LDS and
// shared by the entities of a workgroup, the entities' operands are streamed, and the k-steps above W's diagonal are not walked.
// The selection is mfm_pairs.hpp's (PairsSel, k_pairs_mask, k_pairs_merge), run by k_foldin_rank_select over the written values.
#pragma once
#include "mfm_foldin.hpp"
#include "mfm_pairs.hpp"
#include "mfm_pairs_ucb.hpp"

namespace mfm {

constexpr int FRANK_EB = 8;      // entities of a workgroup: their running moments stay in registers, 4 doubles per entity and lane
constexpr int FRANK_STEP = 256;  // candidates per workgroup step: 64 per wave, one per lane

// ---- the candidate table ------------------------------------------------------------------------------------------------------------
// One workgroup per (64 candidates, sample): foldin_rows_zf forms z and the double-double f of the rows, exactly as for an entity's
// observations; then z goes out in fragment order, Zf[s][c >> 4][k >> 2][(k & 3) * 16 + (c & 15)] (k = component, column =
// candidate: lane l of the MFMA holds B[k l >> 4][col l & 15]), zeros for k >= M and c >= I, and f to F[s][c].
// a: the candidates' CSR in rowptr / colidx / val, and wv, w0, D, K, lin. LDS: foldin_rows_lds_doubles(M).
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin_rank_cand(FoldinArgs a, int64_t I, int64_t Ipad, double *__restrict__ Zf,
                                                                double *__restrict__ F) {
  extern __shared__ double frank_cand_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int off = a.lin, M = a.K + off, ldz = M | 1, KS4 = foldin_keep_ksteps(M);
  const auto [Z, part] = foldin_rows_lds(frank_cand_smem, M);
  const int s = blockIdx.y;
  const int64_t rb = (int64_t)blockIdx.x * FOLDIN_ROWS;
  const int nr = (int)(I - rb < 0 ? 0 : I - rb < FOLDIN_ROWS ? I - rb : FOLDIN_ROWS);
  const double *__restrict__ w = a.wv[s];
  const FoldinDD f = foldin_rows_zf(a, w, w + a.D, a.w0[s], rb, nr, Z, part);
  if (wave == 0) {
    if (off) Z[lane * ldz] = 1.0;
    F[(size_t)s * Ipad + rb + lane] = lane < nr ? f.hi + f.lo : 0.0;
  }
  __syncthreads();
  double *__restrict__ out = Zf + ((size_t)s * (Ipad >> 4) + (rb >> 4)) * KS4 * 64;
  for (int e = tid; e < 4 * KS4 * 64; e += FOLDIN_WG) {
    const int tq = e >> 6, n = tq / KS4, q = tq - n * KS4;
    const int c = n * 16 + (e & 15), k = q * 4 + ((e >> 4) & 3);
    out[e] = (k < M && c < nr) ? Z[c * ldz + k] : 0.0;
  }
}

// ---- the tile kernel ----------------------------------------------------------------------------------------------------------------
struct FoldinRankArgs {
  const double *Wf;     // [Uc][S][RT][KS4][64]: the kept operands of the chunk's entities
  const double *Zf;     // [S][Ipad / 16][KS4][64]
  const double *F;      // [S][Ipad]
  const double *alpha;  // [S]
  int M, KS4, RT, S, nbuf;  // nbuf: LDS stages of z (2 where they fit)
  int64_t Uc, I, Ipad, stripe_len;
  double beta;
  int by_gain;          // the selecting form's value: 0 mean + beta std, 1 gain
  double *mean, *sd, *sd_within, *gain;  // DENSE: [Uc][I] each
  double *value;        // !DENSE: [Uc][I]
};

__host__ __device__ inline size_t frank_stage_doubles(int KS4) { return (size_t)(FRANK_STEP / 16) * KS4 * 64; }

// A workgroup owns FRANK_EB entities x one stripe of candidates and walks the stripe in steps of FRANK_STEP. Per step the samples are
// walked in order; Z_s of the step is copied to LDS once (two stages where they fit: the copy of sample s + 1 by a wave that is
// done overlaps the MFMAs of the others) and serves every entity of the block; per entity a wave streams the operand's
// fragments (512 contiguous bytes per k-step, the same addresses in the four waves) against its own 4 column tiles. Row tile t
// walks the k-steps q < min(KS4, 4 t + 4) only: beyond them W is zero (the tile that holds row M, the mean, walks all of them).
// The tile's rows are squared and summed in the lane (rows < M; row M is m - f), and after the last tile over the four lane
// groups (xor 16, xor 32: every lane ends with the same bits); lane l keeps candidate l of the wave's 64: Welford over m, the
// sums of v and of 1/2 log1p(alpha v), in sample order, in registers. No atomics, nothing summed between workgroups: a result
// depends on the entity's operand and the candidate only (a candidate's lane is its index mod FRANK_STEP).
template <bool DENSE>
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin_rank_tile(FoldinRankArgs a) {
  extern __shared__ double frank_tile_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 4;
  const int M = a.M, KS4 = a.KS4, RT = a.RT, S = a.S;
  const int64_t e0 = (int64_t)blockIdx.x * FRANK_EB;
  const int nE = (int)(a.Uc - e0 < FRANK_EB ? a.Uc - e0 : FRANK_EB);
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  const size_t stage = frank_stage_doubles(KS4), opnd = (size_t)RT * KS4 * 64;
  unsigned it = 0;
  for (int64_t c0 = cb; c0 < ce; c0 += FRANK_STEP) {
    double mean[FRANK_EB], m2[FRANK_EB], sv[FRANK_EB], sg[FRANK_EB];
#pragma unroll
    for (int e = 0; e < FRANK_EB; e++) mean[e] = m2[e] = sv[e] = sg[e] = 0.0;
    const int64_t col = c0 + wave * 64 + lane;  // (< Ipad: the table is padded to whole steps)
    for (int s = 0; s < S; s++, it++) {
      double *buf = frank_tile_smem + (a.nbuf == 2 ? (it & 1) * stage : 0);
      if (a.nbuf == 1) __syncthreads();  // the one stage is still being read
      {
        const double *__restrict__ src = a.Zf + ((size_t)s * (a.Ipad >> 4) + (c0 >> 4)) * KS4 * 64;
        for (size_t i = tid; i < stage; i += FOLDIN_WG) buf[i] = src[i];
      }
      __syncthreads();
      const double *zb = buf + (size_t)wave * 4 * KS4 * 64 + lane;
      const double fcol = a.F[(size_t)s * a.Ipad + col], alpha = a.alpha[s], rn = 1.0 / (double)(s + 1);
#pragma unroll
      for (int e = 0; e < FRANK_EB; e++) {
        if (e >= nE) break;
        const double *__restrict__ wp = a.Wf + ((size_t)(e0 + e) * S + s) * opnd + lane;
        double vp[4] = {0.0, 0.0, 0.0, 0.0}, mp[4] = {0.0, 0.0, 0.0, 0.0};
        for (int t = 0; t < RT; t++) {
          const int qn = KS4 < 4 * t + 4 ? KS4 : 4 * t + 4;
          pairs_d4 acc[4];
#pragma unroll
          for (int n = 0; n < 4; n++) acc[n] = (pairs_d4){0.0, 0.0, 0.0, 0.0};
          const double *__restrict__ wt = wp + (size_t)t * KS4 * 64;
          double an = qn > 0 ? wt[0] : 0.0;
          for (int q = 0; q < qn; q++) {
            const double ac = an;
            if (q + 1 < qn) an = wt[(size_t)(q + 1) * 64];
#pragma unroll
            for (int n = 0; n < 4; n++) acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(ac, zb[((size_t)n * KS4 + q) * 64], acc[n], 0, 0, 0);
          }
          // f64 C/D map: lane l, register g hold (row (l >> 4) + 4 g, column l & 15)
#pragma unroll
          for (int g = 0; g < 4; g++) {
            const int row = t * 16 + grp + 4 * g;
#pragma unroll
            for (int n = 0; n < 4; n++) {
              const double x = acc[n][g];
              if (row < M)
                vp[n] += x * x;
              else if (row == M)
                mp[n] = x;
            }
          }
        }
#pragma unroll
        for (int n = 0; n < 4; n++) {
          vp[n] += __shfl_xor(vp[n], 16);
          vp[n] += __shfl_xor(vp[n], 32);
          mp[n] += __shfl_xor(mp[n], 16);
          mp[n] += __shfl_xor(mp[n], 32);
        }
        const double v = grp == 0 ? vp[0] : grp == 1 ? vp[1] : grp == 2 ? vp[2] : vp[3];
        const double mm = grp == 0 ? mp[0] : grp == 1 ? mp[1] : grp == 2 ? mp[2] : mp[3];
        pairs_welford(fcol + mm, rn, mean[e], m2[e]);
        sv[e] += v;
        sg[e] += 0.5 * log1p(alpha * v);
      }
    }
    if (col < ce) {
#pragma unroll
      for (int e = 0; e < FRANK_EB; e++) {
        if (e >= nE) break;
        const size_t o = (size_t)(e0 + e) * a.I + col;
        const double within2 = sv[e] / (double)S, sd = sqrt(within2 + m2[e] / (double)S), gain = sg[e] / (double)S;
        if constexpr (DENSE) {
          a.mean[o] = mean[e];
          a.sd[o] = sd;
          a.sd_within[o] = sqrt(within2);
          a.gain[o] = gain;
        } else {
          a.value[o] = a.by_gain ? gain : mean[e] + a.beta * sd;
        }
      }
    }
  }
}

// ---- the selection over the written values --------------------------------------------------------------------------------------
// 16 entities x one stripe of a.dense [Uc][I] through PairsSel<1> (mfm_pairs.hpp: threshold, exclusion mask, buffer, compaction,
// the stripe's lists); a round is 64 candidates per row, what a round of the pair scorer appends at most. k_pairs_merge follows.
__global__ __launch_bounds__(PAIRS_WG) void k_foldin_rank_select(PairsArgs a) {
  PairsSel<1> sel;
  sel.init(a.k);
  const int rloc = threadIdx.x >> 4;
  const int64_t q0 = (int64_t)blockIdx.x * 16, row = q0 + rloc;
  const int64_t cb = (int64_t)blockIdx.y * a.stripe_len;
  const int64_t ce = cb + a.stripe_len < a.I ? cb + a.stripe_len : a.I;
  for (int64_t c0 = cb; c0 < ce; c0 += 64) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t col = c0 + (threadIdx.x & 15) + 16 * j;
      if (row < a.Uc && col < ce) sel.push(a, rloc, row, col, a.dense[(size_t)row * a.I + col]);
    }
    sel.round();
  }
  sel.finish(a, q0);
}

// ---- mean, std and gain of the selected entries -----------------------------------------------------------------------------------
// One wave per entry (entity u of the chunk, list position j), as k_pairs_moments_at: lane l takes sample s0 + l and forms W z row
// after row in component order -- not the MFMA's association, so mean + beta std agrees with the selected value within rounding,
// not bit for bit -- then the 64 (m, v) pass through the tile kernel's recurrences in sample order. Index -1: NaN.
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin_rank_at(FoldinRankArgs a, const int32_t *__restrict__ out_i, int k, int64_t n_entries,
                                                              double *__restrict__ out_mean, double *__restrict__ out_sd,
                                                              double *__restrict__ out_gain) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * (FOLDIN_WG / 64) + (threadIdx.x >> 6);
  if (e >= n_entries) return;
  const int64_t u = e / k;
  const int i = out_i[e];
  if (i < 0) {
    if (lane == 0) out_mean[e] = out_sd[e] = out_gain[e] = __builtin_nan("");
    return;
  }
  const int M = a.M, KS4 = a.KS4, S = a.S;
  double mean = 0.0, m2 = 0.0, sv = 0.0, sg = 0.0;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    double m = 0.0, v = 0.0;
    if (s < S) {
      const double *__restrict__ W = a.Wf + ((size_t)u * S + s) * a.RT * KS4 * 64;
      const double *__restrict__ Z = a.Zf + ((size_t)s * (a.Ipad >> 4) + (i >> 4)) * KS4 * 64 + (i & 15);
      for (int r = 0; r <= M; r++) {
        const double *__restrict__ Wr = W + (size_t)(r >> 4) * KS4 * 64 + (r & 15);
        const int kn = r < M ? r + 1 : M;
        double t = 0.0;
        for (int c = 0; c < kn; c++) {
          const int o = (c >> 2) * 64 + (c & 3) * 16;
          t += Wr[o] * Z[o];
        }
        if (r < M)
          v += t * t;
        else
          m = a.F[(size_t)s * a.Ipad + i] + t;
      }
    }
    const int n_here = S - s0 < 64 ? S - s0 : 64;
    for (int j = 0; j < n_here; j++) {
      const double vj = __shfl(v, j);
      pairs_welford(__shfl(m, j), 1.0 / (double)(s0 + j + 1), mean, m2);
      sv += vj;
      sg += 0.5 * log1p(a.alpha[s0 + j] * vj);
    }
  }
  if (lane == 0) {
    out_mean[e] = mean;
    out_sd[e] = sqrt(sv / (double)S + m2 / (double)S);
    out_gain[e] = sg / (double)S;
  }
}

}  // namespace mfm
