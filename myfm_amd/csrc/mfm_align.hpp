// mfm_align.hpp -- the kernels of mfm_align_* (include/myfm_hip.h): orthogonal Procrustes alignment of the kept samples'
// factor matrices. V_s is the (K, D) factor-major matrix of sample s (the store's layout), c the column weights, ref the round's
// reference (a sample, or the previous round's mean). Per round and sample
//   M_s = V_s diag(c) ref^T  (K x K),   R_s = U W^T with M_s = U Sigma W^T,   Y_s = R_s^T V_s,
// mean / std = Welford over s of Y_s. Three kernels, fp64 throughout, no atomics: every sum has one order, fixed by D and K alone.
//   k_align_gram   grid (chunks of ALIGN_CHUNK_TILES * 64 columns) x (groups of ALIGN_GROUP samples): M_s per chunk on
//                  v_mfma_f64_16x16x4_f64, both operands staged coalesced through padded LDS, plus the weighted squared norms
//   k_align_polar  one workgroup per sample: the chunks added in index order, one-sided Jacobi SVD in LDS, R_s and sum sigma_i
//   k_align_apply  one workgroup per 64 columns, all samples in order: Y_s on the MFMA, running mean and M2 in registers
// Neither kernel holds a float: no packed fp32 instruction can be selected for them.
#pragma once
#include "mfm_common.hpp"

#include <type_traits>

namespace mfm {

constexpr int ALIGN_MAX_RANK = 64;
constexpr int ALIGN_WG = 256;
constexpr int ALIGN_TILE = 64;         // columns per staged tile: 512 contiguous bytes per factor row
constexpr int ALIGN_CHUNK_TILES = 32;  // tiles per chunk of k_align_gram: the chunk count depends on D alone
constexpr int ALIGN_GROUP = 4;         // samples per workgroup of k_align_gram: the reference tile is staged once for them
constexpr int ALIGN_LDG = 66;          // row of a staged tile in k_align_gram: lane (row l & 15, column l >> 4) of a half wave -> 4 row + 2 col
constexpr int ALIGN_LDA = 80;          // ... in k_align_apply: lane (column l & 15, row l >> 4) -> 2 col + 32 row
constexpr int ALIGN_LDP = 65;          // column of the K x K matrices of k_align_polar
constexpr int ALIGN_SWEEPS = 30;       // cap of the Jacobi sweeps (a well-conditioned 64 x 64 matrix takes 8 to 10)
constexpr double ALIGN_EPS = 2.220446049250313e-16;   // a pair rotates while |<p, q>| > eps |p| |q|
constexpr double ALIGN_NULL = 1.4551915228366852e-11;  // 2^-36: a column of norm <= this * sigma_max counts as a null column

typedef double align_d4 __attribute__((ext_vector_type(4)));

constexpr int64_t align_chunk_cols() { return (int64_t)ALIGN_CHUNK_TILES * ALIGN_TILE; }
constexpr int align_chunks(int64_t D) { return (int)((D + align_chunk_cols() - 1) / align_chunk_cols()); }
constexpr int align_ldr(int NT) { return (NT & 1) ? NT * 16 : NT * 16 + 16; }  // row of R_s in k_align_apply (16 mod 32 doubles)
constexpr size_t align_gram_lds(int NT) { return (size_t)2 * NT * 16 * ALIGN_LDG * sizeof(double); }
constexpr size_t align_polar_lds() { return (size_t)2 * ALIGN_MAX_RANK * ALIGN_LDP * sizeof(double); }
constexpr size_t align_apply_lds(int NT) { return (size_t)NT * 16 * (ALIGN_LDA + align_ldr(NT)) * sizeof(double); }

// the sum over the wave, every lane the same value: a butterfly, one order whatever the data
__device__ inline double align_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

struct AlignGramArgs {
  const double *const *V = nullptr;  // [S] device pointers: V_s[K][D]
  const double *ref = nullptr;       // [K][D]
  const double *c = nullptr;         // [D], or null: all ones
  int64_t D = 0;
  int K = 0, s0 = 0, ns = 0, nchunks = 0;  // this launch serves samples [s0, s0 + ns)
  double *part = nullptr;                  // [ns][nchunks][K][K]
  double *nv = nullptr;                    // [ns][nchunks]: the chunk's share of |V_s|_c^2
  double *nr = nullptr;                    // [nchunks]: of |ref|_c^2, written by the first group of samples where write_nr
  int write_nr = 0;
};
static_assert(std::is_trivially_copyable<AlignGramArgs>::value, "AlignGramArgs is a kernel argument");

// NT = ceil(K / 16). Thread t owns column t & 63 of every tile and rows (t >> 6) + 4 e, e < 4 NT: a wave's global load is one factor
// row's 512 contiguous bytes. Rows >= K and columns >= D are staged as zeros. The NT^2 output tiles go round robin over the four
// waves (tile n = ta NT + tb to wave n & 3), a sample's accumulators stay in registers over the whole chunk. The next (sample, tile)
// is fetched into registers while the current one is contracted.
template <int NT>
__global__ __launch_bounds__(ALIGN_WG) void k_align_gram(AlignGramArgs a) {
  extern __shared__ double align_smem[];
  __shared__ double s_red[ALIGN_GROUP + 1][4];
  constexpr int NE = 4 * NT, TPW = (NT * NT + 3) / 4;
  double *__restrict__ Rt = align_smem;                  // [16 NT][ALIGN_LDG]: c (.) ref
  double *__restrict__ Vt = Rt + NT * 16 * ALIGN_LDG;    // [16 NT][ALIGN_LDG]: V_s
  const int tid = threadIdx.x, lane = tid & 63, col = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), r0 = tid >> 6;
  const int chunk = blockIdx.x, g0 = blockIdx.y * ALIGN_GROUP;
  const int ng = min(ALIGN_GROUP, a.ns - g0);
  const int64_t dbeg = (int64_t)chunk * align_chunk_cols(), dend = min(a.D, dbeg + align_chunk_cols());
  const int ntiles = (int)((dend - dbeg + ALIGN_TILE - 1) / ALIGN_TILE);

  const double *Vp[ALIGN_GROUP];
#pragma unroll
  for (int g = 0; g < ALIGN_GROUP; g++) Vp[g] = a.V[a.s0 + g0 + (g < ng ? g : 0)];
  align_d4 acc[ALIGN_GROUP][TPW];
  double nv[ALIGN_GROUP], nr = 0.0, nx[NE];
#pragma unroll
  for (int g = 0; g < ALIGN_GROUP; g++) {
    nv[g] = 0.0;
#pragma unroll
    for (int t = 0; t < TPW; t++) acc[g][t] = (align_d4){0.0, 0.0, 0.0, 0.0};
  }
  const auto fetch = [&](const double *__restrict__ src, int64_t d0) {
    // (the column clamped and zeroed when staged; rows in fours, the tests on 4 e the same for every thread: no predicate lives
    // across the MFMAs, one pointer steps down the rows)
    const double *__restrict__ q = src + (int64_t)r0 * a.D + min(d0 + col, a.D - 1);
#pragma unroll
    for (int e = 0; e < NE; e++) {
      if (4 * e + 3 < a.K)
        nx[e] = *q;
      else if (4 * e < a.K)
        nx[e] = r0 + 4 * e < a.K ? *q : 0.0;
      else
        nx[e] = 0.0;
      q += 4 * a.D;
    }
  };
  fetch(Vp[0], dbeg);
  const int aoff = (lane & 15) * ALIGN_LDG + (lane >> 4);
  for (int t = 0; t < ntiles; t++) {
    const int64_t d0 = dbeg + (int64_t)t * ALIGN_TILE, d = d0 + col;
    const double cv = d < a.D ? (a.c ? a.c[d] : 1.0) : 0.0;
#pragma unroll
    for (int g = 0; g < ALIGN_GROUP; g++) {
      if (g >= ng) continue;  // (the same for the whole workgroup)
      __syncthreads();
      if (g == 0) {
#pragma unroll
        for (int e = 0; e < NE; e++) {
          const int row = r0 + 4 * e;
          const double x = row < a.K && d < a.D ? a.ref[(int64_t)row * a.D + d] : 0.0, cx = cv * x;
          Rt[row * ALIGN_LDG + col] = cx;
          nr += cx * x;
        }
      }
#pragma unroll
      for (int e = 0; e < NE; e++) {
        const double x = d < a.D ? nx[e] : 0.0;
        Vt[(r0 + 4 * e) * ALIGN_LDG + col] = x;
        nv[g] += (cv * x) * x;
      }
      __syncthreads();
      if (g + 1 < ng)
        fetch(Vp[(g + 1) & (ALIGN_GROUP - 1)], d0);
      else if (t + 1 < ntiles)
        fetch(Vp[0], d0 + ALIGN_TILE);
#pragma unroll 4
      for (int j = 0; j < ALIGN_TILE / 4; j++)
#pragma unroll
        for (int tt = 0; tt < TPW; tt++) {
          const int n = wave + 4 * tt;
          if (n < NT * NT) {
            const double A = Vt[(n / NT) * 16 * ALIGN_LDG + aoff + 4 * j];
            const double B = Rt[(n % NT) * 16 * ALIGN_LDG + aoff + 4 * j];
            acc[g][tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, acc[g][tt], 0, 0, 0);
          }
        }
    }
  }
  // ---- the partials (f64 C/D map: lane l, register r hold (row (l >> 4) + 4 r, column l & 15)) and the norms
#pragma unroll
  for (int g = 0; g < ALIGN_GROUP; g++) {
    if (g >= ng) continue;
    double *__restrict__ out = a.part + ((size_t)(g0 + g) * a.nchunks + chunk) * a.K * a.K;
#pragma unroll
    for (int tt = 0; tt < TPW; tt++) {
      const int n = wave + 4 * tt;
      if (n < NT * NT)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int ra = (n / NT) * 16 + (lane >> 4) + 4 * r, cb = (n % NT) * 16 + (lane & 15);
          if (ra < a.K && cb < a.K) out[ra * a.K + cb] = acc[g][tt][r];
        }
    }
    const double w = align_wave_sum(nv[g]);
    if (lane == 0) s_red[g][wave] = w;
  }
  const double wr = align_wave_sum(nr);
  if (lane == 0) s_red[ALIGN_GROUP][wave] = wr;
  __syncthreads();
  if (tid < ng) a.nv[(size_t)(g0 + tid) * a.nchunks + chunk] = ((s_red[tid][0] + s_red[tid][1]) + s_red[tid][2]) + s_red[tid][3];
  if (tid == 0 && a.write_nr && blockIdx.y == 0)
    a.nr[chunk] = ((s_red[ALIGN_GROUP][0] + s_red[ALIGN_GROUP][1]) + s_red[ALIGN_GROUP][2]) + s_red[ALIGN_GROUP][3];
}

struct AlignPolarArgs {
  const double *part = nullptr, *nv = nullptr, *nr = nullptr;  // k_align_gram's, of samples [s0, s0 + gridDim.x)
  int K = 0, nchunks = 0, s0 = 0;
  double *R = nullptr;      // [S][K][K]
  double *align = nullptr;  // [S]
};
static_assert(std::is_trivially_copyable<AlignPolarArgs>::value, "AlignPolarArgs is a kernel argument");

// One workgroup per sample. A (LDS, column-major: column p at A + p ALIGN_LDP) starts as M_s, W as I; a Jacobi rotation of the
// column pair (p, q) is applied to both, so M_s W = A throughout and at the end A = U Sigma. The pairs of a step come from the
// round-robin (circle) schedule over Kk = K + (K & 1) players, Kk - 1 steps per sweep, player K of an odd K the bye; a pair is owned
// by 8 lanes, which split the rows. A pair whose inner product is exactly 0 is left alone. Null columns (norm <= ALIGN_NULL
// sigma_max, a zero matrix included) are replaced on wave 0: for each in index order, the first unit vector e_i whose residual
// against the columns set so far is at least 1 / (2 K) of its length squared (one exists: the residuals sum to K minus the number
// set) is orthogonalised against them twice and normalised. R_s[a][b] = sum_j U[a][j] W[b][j].
__global__ __launch_bounds__(ALIGN_WG) void k_align_polar(AlignPolarArgs a) {
  extern __shared__ double align_smem[];
  __shared__ double s_sig[ALIGN_MAX_RANK];
  __shared__ double s_norm[2];
  const int K = a.K, tid = threadIdx.x, lane = tid & 63;
  const int s = blockIdx.x;
  double *__restrict__ A = align_smem;
  double *__restrict__ W = A + ALIGN_MAX_RANK * ALIGN_LDP;
  for (int idx = tid; idx < K * K; idx += ALIGN_WG) {
    const int ra = idx / K, cb = idx - ra * K;
    double m = 0.0;
    for (int ch = 0; ch < a.nchunks; ch++) m += a.part[((size_t)s * a.nchunks + ch) * K * K + idx];
    A[cb * ALIGN_LDP + ra] = m;
    W[cb * ALIGN_LDP + ra] = ra == cb ? 1.0 : 0.0;
  }
  if (tid < 2) {
    double m = 0.0;
    for (int ch = 0; ch < a.nchunks; ch++) m += tid == 0 ? a.nv[(size_t)s * a.nchunks + ch] : a.nr[ch];
    s_norm[tid] = m;
  }
  __syncthreads();

  // ---- one-sided Jacobi
  const int Kk = K + (K & 1), np = Kk >> 1, m1 = Kk - 1;
  const int pair = tid >> 3, sub = tid & 7;
  for (int sweep = 0; sweep < ALIGN_SWEEPS; sweep++) {
    int any = 0;
    for (int step = 0; step < m1; step++) {
      int p = (step + pair) % m1, q = pair == 0 ? m1 : (step + m1 - pair) % m1;
      if (p > q) {
        const int t = p;
        p = q;
        q = t;
      }
      const bool valid = pair < np && q < K;
      double al = 0.0, be = 0.0, ga = 0.0;
      if (valid)
        for (int r = sub; r < K; r += 8) {
          const double x = A[p * ALIGN_LDP + r], y = A[q * ALIGN_LDP + r];
          al += x * x;
          be += y * y;
          ga += x * y;
        }
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) {
        al += __shfl_xor(al, off);
        be += __shfl_xor(be, off);
        ga += __shfl_xor(ga, off);
      }
      const bool rot = valid && ga != 0.0 && fabs(ga) > ALIGN_EPS * (sqrt(al) * sqrt(be));
      if (rot) {
        const double zeta = (be - al) / (2.0 * ga);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
        for (int r = sub; r < K; r += 8) {
          const double x = A[p * ALIGN_LDP + r], y = A[q * ALIGN_LDP + r];
          A[p * ALIGN_LDP + r] = c * x - sn * y;
          A[q * ALIGN_LDP + r] = sn * x + c * y;
          const double wx = W[p * ALIGN_LDP + r], wy = W[q * ALIGN_LDP + r];
          W[p * ALIGN_LDP + r] = c * wx - sn * wy;
          W[q * ALIGN_LDP + r] = sn * wx + c * wy;
        }
      }
      any |= __syncthreads_or(rot ? 1 : 0);
    }
    if (!any) break;
  }

  // ---- sigma, U = A / sigma
  if (tid < K) {
    double sq = 0.0;
    for (int r = 0; r < K; r++) sq += A[tid * ALIGN_LDP + r] * A[tid * ALIGN_LDP + r];
    s_sig[tid] = sqrt(sq);
  }
  __syncthreads();
  double smax = 0.0, ssum = 0.0;
  for (int j = 0; j < K; j++) {
    smax = fmax(smax, s_sig[j]);
    ssum += s_sig[j];
  }
  const double thr = ALIGN_NULL * smax;
  unsigned long long set = 0;  // (K <= 64) the columns that hold a unit vector
  for (int j = 0; j < K; j++)
    if (s_sig[j] > thr) set |= 1ull << j;
  for (int idx = tid; idx < K * K; idx += ALIGN_WG) {
    const int j = idx / K, r = idx - j * K;
    if ((set >> j) & 1) A[j * ALIGN_LDP + r] /= s_sig[j];
  }
  __syncthreads();
  const unsigned long long full = K == 64 ? ~0ull : (1ull << K) - 1;
  if (set != full) {
    if (tid < 64) {  // wave 0, lane = row
      const bool live = lane < K;
      for (int j = 0; j < K; j++) {
        if ((set >> j) & 1) continue;
        double res = 1.0;
        for (int u = 0; u < K; u++)
          if ((set >> u) & 1) {
            const double x = live ? A[u * ALIGN_LDP + lane] : 0.0;
            res -= x * x;
          }
        const unsigned long long ok = __ballot(live && res >= 0.5 / (double)K);
        const int pick = ok ? __ffsll((long long)ok) - 1 : 0;
        double v = lane == pick ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++)
          for (int u = 0; u < K; u++)
            if ((set >> u) & 1) {
              const double x = live ? A[u * ALIGN_LDP + lane] : 0.0;
              const double dot = align_wave_sum(v * x);
              v -= dot * x;
            }
        const double nrm = sqrt(align_wave_sum(v * v));
        if (live) A[j * ALIGN_LDP + lane] = v / nrm;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        set |= 1ull << j;
      }
    }
    __syncthreads();
  }

  // ---- R = U W^T, the alignment
  double *__restrict__ R = a.R + (size_t)(a.s0 + s) * K * K;
  for (int idx = tid; idx < K * K; idx += ALIGN_WG) {
    const int ra = idx / K, cb = idx - ra * K;
    double m = 0.0;
    for (int j = 0; j < K; j++) m += A[j * ALIGN_LDP + ra] * W[j * ALIGN_LDP + cb];
    R[idx] = m;
  }
  if (tid == 0) {
    const double nv = s_norm[0], nr = s_norm[1];
    double den = sqrt(nv * nr);  // (exact where the norms are: sqrt(nv) sqrt(nr) is not)
    if (!(den > 0.0) || !(den < INFINITY)) den = sqrt(nv) * sqrt(nr);
    a.align[a.s0 + s] = nv > 0.0 && nr > 0.0 ? fmin(ssum / den, 1.0) : 0.0;
  }
}

struct AlignApplyArgs {
  const double *const *V = nullptr;  // [S] device pointers: V_s[K][D]
  const double *R = nullptr;         // [S][K][K]
  int64_t D = 0;
  int K = 0, S = 0;
  double *mean = nullptr, *std = nullptr;  // [K][D]
};
static_assert(std::is_trivially_copyable<AlignApplyArgs>::value, "AlignApplyArgs is a kernel argument");

// One workgroup per tile of 64 columns, the samples in order. MFMA A[d][a] = V_s[a][d] (lane (d = l & 15, a = l >> 4) reads the
// staged tile along d), B[a][b] = R_s[a][b]; wave w owns columns [16 w, 16 w + 16) of the tile and all NT b-tiles, so Y, the running
// mean and M2 are NT x 4 doubles each per lane. Welford in sample order: delta = y - mean, mean += delta / n, M2 += delta (y - mean).
// The next sample's tile and rotation are fetched into registers while the current one is contracted. mean and std leave through the
// staged tile's LDS, so that the global stores run along d.
template <int NT>
__global__ __launch_bounds__(ALIGN_WG) void k_align_apply(AlignApplyArgs a) {
  extern __shared__ double align_smem[];
  constexpr int NE = 4 * NT, NR = NT * NT, KP = NT * 16, LDR = align_ldr(NT);
  double *__restrict__ Vt = align_smem;          // [KP][ALIGN_LDA]
  double *__restrict__ Rl = Vt + KP * ALIGN_LDA;  // [KP][LDR]
  const int tid = threadIdx.x, lane = tid & 63, col = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), r0 = tid >> 6;
  const int64_t d0 = (int64_t)blockIdx.x * ALIGN_TILE, d = d0 + col;
  double nxv[NE], nxr[NR];
  const auto fetch = [&](int s) {
    const double *__restrict__ src = a.V[s];
    const double *__restrict__ R = a.R + (size_t)s * a.K * a.K;
    const double *__restrict__ q = src + (int64_t)r0 * a.D + min(d, a.D - 1);  // (as k_align_gram's fetch)
#pragma unroll
    for (int e = 0; e < NE; e++) {
      if (4 * e + 3 < a.K)
        nxv[e] = *q;
      else if (4 * e < a.K)
        nxv[e] = r0 + 4 * e < a.K ? *q : 0.0;
      else
        nxv[e] = 0.0;
      q += 4 * a.D;
    }
#pragma unroll
    for (int e = 0; e < NR; e++) {
      const int idx = tid + ALIGN_WG * e;
      nxr[e] = R[min(idx / KP, a.K - 1) * a.K + min(idx % KP, a.K - 1)];
    }
  };
  align_d4 mean[NT], m2[NT];
#pragma unroll
  for (int bt = 0; bt < NT; bt++) mean[bt] = m2[bt] = (align_d4){0.0, 0.0, 0.0, 0.0};
  fetch(0);
  for (int s = 0; s < a.S; s++) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NE; e++) Vt[(r0 + 4 * e) * ALIGN_LDA + col] = d < a.D ? nxv[e] : 0.0;
#pragma unroll
    for (int e = 0; e < NR; e++) {
      const int idx = tid + ALIGN_WG * e;
      Rl[(idx / KP) * LDR + idx % KP] = idx / KP < a.K && idx % KP < a.K ? nxr[e] : 0.0;
    }
    __syncthreads();
    if (s + 1 < a.S) fetch(s + 1);
    align_d4 y[NT];
#pragma unroll
    for (int bt = 0; bt < NT; bt++) y[bt] = (align_d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int j = 0; j < KP / 4; j++) {
      const double A = Vt[(4 * j + (lane >> 4)) * ALIGN_LDA + wave * 16 + (lane & 15)];
#pragma unroll
      for (int bt = 0; bt < NT; bt++) {
        const double B = Rl[(4 * j + (lane >> 4)) * LDR + bt * 16 + (lane & 15)];
        y[bt] = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, y[bt], 0, 0, 0);
      }
    }
    const double n = (double)(s + 1);
#pragma unroll
    for (int bt = 0; bt < NT; bt++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double delta = y[bt][r] - mean[bt][r];
        mean[bt][r] += delta / n;
        m2[bt][r] += delta * (y[bt][r] - mean[bt][r]);
      }
  }
  // ---- out (f64 C/D map: lane l, register r hold (d = 16 w + (l >> 4) + 4 r, b = 16 bt + (l & 15)))
  const double nS = (double)a.S;
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    __syncthreads();
#pragma unroll
    for (int bt = 0; bt < NT; bt++)
#pragma unroll
      for (int r = 0; r < 4; r++)
        Vt[(bt * 16 + (lane & 15)) * ALIGN_LDA + wave * 16 + (lane >> 4) + 4 * r] = pass == 0 ? mean[bt][r] : sqrt(m2[bt][r] / nS);
    __syncthreads();
    double *__restrict__ out = pass == 0 ? a.mean : a.std;
#pragma unroll
    for (int e = 0; e < NE; e++) {
      const int row = r0 + 4 * e;
      if (row < a.K && d < a.D) out[(int64_t)row * a.D + d] = Vt[row * ALIGN_LDA + col];
    }
  }
}

}  // namespace mfm
