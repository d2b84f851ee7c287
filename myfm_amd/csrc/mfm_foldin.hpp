// mfm_foldin.hpp -- the kernel of mfm_foldin_* (mfm_foldin.hip): the exact conditional posterior of the parameters of a
// NEW one-hot feature u (a user or an item that was not in the training table) under one kept sample. With value 1 in its rows the
// feature enters the score linearly,
//   score_s(x + e_u) = f_s(x) + w_u + sum_k V_uk q_sk(x),   q_sk(x) = sum_j V_s[k, j] x_j      (the -1/2 V_uk^2 self term cancels),
// so theta_u = (w_u, V_u1 .. V_uK) has a Gaussian posterior of dimension M = K + 1 (M = K for a model fitted without the linear term):
//   Lambda = diag(lambda) + alpha sum_i z_i z_i^T,   b = diag(lambda) mu + alpha sum_i z_i r_i,   z_i = (1, q_s(x_i)),  r_i = y_i - f_s(x_i)
//   theta_mean = Lambda^-1 b,   a draw: theta_mean + L^-T eps with Lambda = L L^T.
// One workgroup owns one (entity, sample). It walks the entity's rows in passes of FOLDIN_ROWS: lane l of every wave forms row l's
// q (wave w the factors w, w + 4, ..: a gather for one factor stays inside that factor's D-long vector of the factor-major store), f and
// the residual (f in double-double, see there) into LDS; then every thread adds the pass to its entries of the upper triangle of the Gram matrix and of b, in row
// order. Nothing is summed between workgroups and no order depends on the grid: a result depends on the entity's own rows only, not on
// the number of entities, the chunking or the scratch bound. The factorisation and the two triangular solves run in LDS.
#pragma once
#include "mfm_common.hpp"
#include "mfm_philox.hpp"

namespace mfm {

constexpr int FOLDIN_WG = 256;      // 4 waves
constexpr int FOLDIN_ROWS = 64;     // rows of an entity per pass: one per lane
constexpr int FOLDIN_MAX_RANK = 64; // (K + 1)^2 + 64 (K + 1) doubles of LDS: 77 KB at rank 64, two workgroups per CU
// the draw index of the per-row Philox stream (mfm_philox.hpp) that the posterior draws use: stream (seed, this, row = s U + u).
// The latent draws of the probit tasks use the iteration number there; "FOLDIN" in ASCII is out of their reach.
constexpr uint64_t FOLDIN_DRAW_TAG = 0x464F4C44494Eull;

struct FoldinArgs {
  const int64_t *rowptr;   // the context rows, grouped by entity: CSR in the model's feature space
  const int32_t *colidx;
  const double *val, *y;
  const int64_t *eoff;     // [U + 1]: entity u owns rows [eoff[u], eoff[u + 1])
  const double *const *wv; // per sample of the call: w[D] then V[K][D]
  const double *w0;        // [S]
  const double *alpha;     // [S]
  const double *mu, *lam;  // [S][K + 1]: component 0 the linear weight's, 1 + k factor k's
  int64_t D, U;            // U: all entities of the handle (the stream's row is s U + u)
  int64_t u0;              // this launch: entities [u0, u0 + gridDim.x), samples [s0, s0 + gridDim.y)
  int s0, K, lin;          // lin: the model has a linear term (M = K + lin)
  uint64_t seed;
  double *out_w, *out_V;   // [gridDim.y][gridDim.x], [gridDim.y][gridDim.x][K]
  int *err;                // set when a pivot is not positive
};

// doubles of dynamic LDS before the (i, j) table of the upper triangle
__host__ __device__ inline size_t foldin_lds_doubles(int M) {
  const size_t ldz = (size_t)M | 1;
  return (size_t)M * M + M + FOLDIN_ROWS * ldz + FOLDIN_ROWS + 2 * (FOLDIN_WG / 64) * FOLDIN_ROWS;
}
__host__ __device__ inline size_t foldin_lds_bytes(int M) {
  return foldin_lds_doubles(M) * sizeof(double) + ((size_t)M * (M + 1) / 2) * sizeof(uint16_t) + 16;
}

// an unevaluated sum hi + lo, |lo| <= ulp(hi) / 2: add() takes a term given the same way (Knuth's two-sum; the unit is compiled
// without contraction, so every operation below rounds once)
struct FoldinDD {
  double hi = 0.0, lo = 0.0;
  __device__ __forceinline__ void add(double th, double tl) {
    const double s = hi + th, bb = s - hi;
    const double e = (hi - (s - bb)) + (th - bb);
    const double l = lo + (e + tl);
    hi = s + l;
    lo = l - (hi - s);
  }
};

// z and f of rows [rb, rb + nr) of the context table under the sample (w0, w, V): lane = row, wave w the factors w, w + 4, ...
// Z[lane][off + k] takes q_k of row `lane` (the caller sets column 0 where the model has a linear term); wave 0 returns the row's
// f in double-double, the other waves an empty sum. One barrier inside; the caller places one more before Z is read.
__device__ __forceinline__ FoldinDD foldin_rows_zf(const FoldinArgs &a, const double *__restrict__ w, const double *__restrict__ V,
                                                   double w0, int64_t rb, int nr, double *Z, double *part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K, off = a.lin, ldz = (K + off) | 1;
  int64_t pb = 0, pe = 0;
  if (lane < nr) {
    pb = a.rowptr[rb + lane];
    pe = a.rowptr[rb + lane + 1];
  }
  // f in double-double. The posterior is driven by the residual r = y - f, which is of the noise's size while y and f are of
  // the target's: an error of one rounding of f's TERMS in r moves theta by alpha z / Lambda times that, which a bound relative
  // to |theta| does not cover for an entity with one or two rows. The pair term is taken as sum_{p' < p} t_p t_p' (t_p = x_p v_p,
  // a running prefix sum) instead of 1/2 (q^2 - sum t^2): no cancellation, and exactly 0 for a one-hot row.
  FoldinDD lin, pair;
  if (wave == 0)
    for (int64_t p = pb; p < pe; p++) {
      const double x = a.val[p], wj = w[a.colidx[p]];
      const double ph = x * wj;
      lin.add(ph, fma(x, wj, -ph));
    }
  for (int k = wave; k < K; k += FOLDIN_WG / 64) {
    const double *__restrict__ Vk = V + (int64_t)k * a.D;
    FoldinDD q;
    for (int64_t p = pb; p < pe; p++) {
      const double x = a.val[p], v = Vk[a.colidx[p]];
      const double th = x * v, tl = fma(x, v, -th);  // t = th + tl exactly
      const double ph = th * q.hi;
      pair.add(ph, fma(th, q.hi, -ph) + (th * q.lo + tl * q.hi));
      q.add(th, tl);
    }
    Z[lane * ldz + off + k] = q.hi + q.lo;
  }
  if (wave == 0) pair.add(lin.hi, lin.lo);
  part[wave * FOLDIN_ROWS + lane] = pair.hi;
  part[(FOLDIN_WG / 64 + wave) * FOLDIN_ROWS + lane] = pair.lo;
  __syncthreads();
  FoldinDD f;
  if (wave == 0) {
    f.add(w0, 0.0);
#pragma unroll
    for (int q = 0; q < FOLDIN_WG / 64; q++) f.add(part[q * FOLDIN_ROWS + lane], part[(FOLDIN_WG / 64 + q) * FOLDIN_ROWS + lane]);
  }
  return f;
}

template <bool DRAW>
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin(FoldinArgs a) {
  extern __shared__ double foldin_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, off = a.lin, M = K + off, ldz = M | 1;
  const int T = M * (M + 1) / 2;
  double *A = foldin_smem;                    // [M][M], the upper triangle: the Gram sums, then Lambda, then U = L^T
  double *bv = A + M * M;                     // [M]: sum z r, then b, then the solves' right-hand side
  double *Z = bv + M;                         // [FOLDIN_ROWS][ldz]: the pass's z (ldz odd: a column walk touches every bank)
  double *res = Z + FOLDIN_ROWS * ldz;        // [FOLDIN_ROWS]: the pass's residuals
  double *part = res + FOLDIN_ROWS;           // [2][4][FOLDIN_ROWS]: per wave the high and low parts of its factors' pair terms
  uint16_t *tab = (uint16_t *)(part + 2 * (FOLDIN_WG / 64) * FOLDIN_ROWS);  // [T]: i | j << 8 of triangle entry e

  const int64_t u = a.u0 + blockIdx.x;
  const int sl = blockIdx.y, s = a.s0 + sl;
  const double *__restrict__ w = a.wv[s];
  const double *__restrict__ V = w + a.D;
  const double *__restrict__ mu = a.mu + (size_t)s * (K + 1) + (1 - off);
  const double *__restrict__ lam = a.lam + (size_t)s * (K + 1) + (1 - off);
  const double alpha = a.alpha[s], w0 = a.w0[s];
  const int64_t e0 = a.eoff[u], e1 = a.eoff[u + 1];
  double *__restrict__ ow = a.out_w + (size_t)sl * gridDim.x + blockIdx.x;
  double *__restrict__ oV = a.out_V + ((size_t)sl * gridDim.x + blockIdx.x) * K;

  // the draw's normals: component j is the Box-Muller value of counter word j >> 1, r cos for even j, r sin for odd j
  double eps = 0.0;
  if (DRAW && tid < M) {
    const int64_t srow = (int64_t)s * a.U + u;
    RowRng g(a.seed ^ ((uint64_t)(srow >> 32) * 0x9E3779B97F4A7C15ull), FOLDIN_DRAW_TAG, (uint32_t)srow);
    g.n = (uint32_t)(tid >> 1);
    const double2 un = g.next2();
    const double r = sqrt(-2.0 * log(un.x));
    double sn, cs;
    sincospi(2.0 * un.y, &sn, &cs);
    eps = (tid & 1) ? r * sn : r * cs;
  }

  if (e1 == e0) {  // no rows: the prior itself, mu bit for bit (the factorisation would round lambda mu / sqrt(lambda) / sqrt(lambda))
    if (tid < M) {
      double t = mu[tid];
      if (DRAW) t = t + eps / sqrt(lam[tid]);
      if (off && tid == 0)
        *ow = t;
      else
        oV[tid - off] = t;
    }
    if (!off && tid == 0) *ow = 0.0;
    return;
  }

  for (int t = tid; t < M * M; t += FOLDIN_WG) {
    const int i = t / M, j = t - i * M;
    A[t] = 0.0;
    if (i <= j) tab[i * M - (i * (i - 1)) / 2 + (j - i)] = (uint16_t)(i | (j << 8));
  }
  for (int t = tid; t < M; t += FOLDIN_WG) bv[t] = 0.0;
  __syncthreads();

  for (int64_t rb = e0; rb < e1; rb += FOLDIN_ROWS) {
    const int nr = (int)(e1 - rb < FOLDIN_ROWS ? e1 - rb : FOLDIN_ROWS);
    // ---- z, f and the residual of rows [rb, rb + nr)
    {
      const FoldinDD f = foldin_rows_zf(a, w, V, w0, rb, nr, Z, part);
      if (wave == 0) {
        double rr = 0.0;
        if (lane < nr) {
          const double yv = a.y[rb + lane];
          const double d = yv - f.hi, bb = d - yv;  // two-sum of y and -f.hi
          rr = d + (((yv - (d - bb)) + (-f.hi - bb)) - f.lo);
        }
        res[lane] = rr;
        if (off) Z[lane * ldz] = 1.0;
      }
      __syncthreads();
    }
    // ---- the pass's share of sum z z^T (upper triangle) and of sum z r, row after row
    for (int e = tid; e < T + M; e += FOLDIN_WG) {
      if (e < T) {
        const int ij = tab[e], i = ij & 255, j = ij >> 8;
        double acc = A[i * M + j];
        for (int r = 0; r < nr; r++) acc = fma(Z[r * ldz + i], Z[r * ldz + j], acc);
        A[i * M + j] = acc;
      } else {
        const int i = e - T;
        double acc = bv[i];
        for (int r = 0; r < nr; r++) acc = fma(Z[r * ldz + i], res[r], acc);
        bv[i] = acc;
      }
    }
    __syncthreads();
  }

  // ---- Lambda and b
  for (int e = tid; e < T + M; e += FOLDIN_WG) {
    if (e < T) {
      const int ij = tab[e], i = ij & 255, j = ij >> 8;
      const double g = alpha * A[i * M + j];
      A[i * M + j] = i == j ? lam[i] + g : g;
    } else {
      const int i = e - T;
      bv[i] = fma(lam[i], mu[i], alpha * bv[i]);
    }
  }
  __syncthreads();

  // ---- Lambda = U^T U in place (right-looking; every entry takes its updates in column order)
  bool bad = false;
  for (int j = 0; j < M; j++) {
    const double d = A[j * M + j];  // (the same value in every thread: the exit is uniform)
    if (!(d > 0.0) || !(d < INFINITY)) {
      bad = true;
      break;
    }
    const double piv = sqrt(d);
    __syncthreads();
    for (int i = j + tid; i < M; i += FOLDIN_WG) A[j * M + i] = i == j ? piv : A[j * M + i] / piv;
    __syncthreads();
    const int m = M - j - 1;
    for (int t = tid; t < m * m; t += FOLDIN_WG) {
      const int i = j + 1 + t / m, k = j + 1 + t % m;
      if (i <= k) A[i * M + k] = fma(-A[j * M + i], A[j * M + k], A[i * M + k]);
    }
    __syncthreads();
  }
  if (bad) {  // a non-finite or non-positive lambda: reported through the handle, never a NaN in the result
    if (tid == 0) atomicOr(a.err, 1);
    if (tid < M) {
      if (off && tid == 0)
        *ow = 0.0;
      else
        oV[tid - off] = 0.0;
    }
    if (!off && tid == 0) *ow = 0.0;
    return;
  }

  // ---- U^T yv = b (forward, column-oriented), then U theta = yv (+ eps for a draw: theta_mean + U^-1 eps in one solve)
  for (int j = 0; j < M; j++) {
    const double yj = bv[j] / A[j * M + j];
    __syncthreads();
    if (tid == 0) bv[j] = yj;
    for (int i = j + 1 + tid; i < M; i += FOLDIN_WG) bv[i] = fma(-A[j * M + i], yj, bv[i]);
    __syncthreads();
  }
  if (DRAW) {
    if (tid < M) bv[tid] += eps;
    __syncthreads();
  }
  for (int j = M - 1; j >= 0; j--) {
    const double tj = bv[j] / A[j * M + j];
    __syncthreads();
    if (tid == 0) bv[j] = tj;
    for (int i = tid; i < j; i += FOLDIN_WG) bv[i] = fma(-A[i * M + j], tj, bv[i]);
    __syncthreads();
  }
  if (tid < M) {
    if (off && tid == 0)
      *ow = bv[0];
    else
      oV[tid - off] = bv[tid];
  }
  if (!off && tid == 0) *ow = 0.0;
}

}  // namespace mfm
