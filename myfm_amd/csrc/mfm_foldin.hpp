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
// The steps that the probit chain (k_foldin_gibbs, mfm_foldin_gibbs.hpp) takes in the same way are said once here: the LDS layout
// (foldin_lds), the cell and the write of theta (FoldinCell), the Gram sums (foldin_gram_*), the factorisation (foldin_factor) and
// the draw's normals (foldin_normal).
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
  double *Wf = nullptr;    // KEEP: [gridDim.x][S_all][foldin_keep_doubles(M)], the left operands of mfm_foldin_rank.hpp
  int S_all = 0;           // KEEP: samples of the call (an entity's operands lie sample after sample)
};

// The kept factor of one (entity, sample), KEEP: W = U^-T (lower triangular, M x M; z^T Lambda^-1 z = |W z|^2) and below it
// theta_mean^T as row M, an (M + 1) x M left operand in the fragment order of v_mfma_f64_16x16x4_f64 (the layout k_pairs_embed
// writes, mfm_pairs.hpp): 16-row tiles x 4-wide k-steps, the 64 values of (tile t, k-step q) contiguous, (row r, component k) at
// (k & 3) * 16 + (r & 15); rows above M and components from M on are zeros.
__host__ __device__ inline int foldin_keep_tiles(int M) { return (M + 16) >> 4; }  // row tiles of the M + 1 rows
__host__ __device__ inline int foldin_keep_ksteps(int M) { return (M + 3) >> 2; }
__host__ __device__ inline size_t foldin_keep_doubles(int M) { return (size_t)foldin_keep_tiles(M) * foldin_keep_ksteps(M) * 64; }

// ---- the dynamic LDS of a workgroup: layout and size side by side ------------------------------------------------------------------
// What foldin_rows_zf fills, which is all that k_foldin_rank_cand (mfm_foldin_rank.hpp) asks for
struct FoldinRowsLds {
  double *Z;     // [FOLDIN_ROWS][ldz]: the pass's z (ldz = M | 1 is odd: a column walk touches every bank)
  double *part;  // [2][4][FOLDIN_ROWS]: per wave the high and low parts of its factors' pair terms
};
__host__ __device__ inline size_t foldin_rows_lds_doubles(int M) {
  return FOLDIN_ROWS * ((size_t)M | 1) + 2 * (FOLDIN_WG / 64) * FOLDIN_ROWS;
}
__device__ __forceinline__ FoldinRowsLds foldin_rows_lds(double *smem, int M) { return {smem, smem + FOLDIN_ROWS * (M | 1)}; }

// A cell's (k_foldin, k_foldin_gibbs): the matrix, the right-hand side and the residuals before the rows' part, the table behind it
struct FoldinLds {
  double *A;      // [M][M], the upper triangle: the Gram sums, then Lambda, then U = L^T
  double *bv;     // [M]: sum z r, then b, then the solves' right-hand side
  double *res;    // [FOLDIN_ROWS]: the pass's residuals
  double *Z, *part;
  uint16_t *tab;  // [T]: i | j << 8 of entry e of the upper triangle, T = M (M + 1) / 2
};
// doubles before tab
__host__ __device__ inline size_t foldin_lds_doubles(int M) { return (size_t)M * M + M + FOLDIN_ROWS + foldin_rows_lds_doubles(M); }
__host__ __device__ inline size_t foldin_lds_bytes(int M) {
  return foldin_lds_doubles(M) * sizeof(double) + ((size_t)M * (M + 1) / 2) * sizeof(uint16_t) + 16;
}
__device__ __forceinline__ FoldinLds foldin_lds(double *smem, int M) {
  double *bv = smem + M * M, *res = bv + M;
  const FoldinRowsLds r = foldin_rows_lds(res + FOLDIN_ROWS, M);
  return {smem, bv, res, r.Z, r.part, (uint16_t *)(smem + foldin_lds_doubles(M))};
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

// ---- the steps of a cell that the closed form and the probit chain share ------------------------------------------------------------
// The cell of workgroup (blockIdx.x, blockIdx.y): entity u under sample s of the call, the sample's model and prior (component 0 of
// mu / lam is passed over without a linear term), the entity's rows [e0, e1), the cell's outputs and its row of the draws' streams.
struct FoldinCell {
  int64_t u, e0, e1, srow;
  int sl, s, off, M;
  const double *w, *V, *mu, *lam;
  double w0;
  double *ow, *oV;
  // v: component threadIdx.x of theta (read below M only). Component 0 is w where the model has a linear term, which is 0 otherwise.
  __device__ __forceinline__ void put(double v) const {
    const int tid = threadIdx.x;
    if (tid < M) {
      if (off && tid == 0)
        *ow = v;
      else
        oV[tid - off] = v;
    }
    if (!off && tid == 0) *ow = 0.0;
  }
  // a cell without a result: reported through the handle, never a NaN in the output
  __device__ __forceinline__ void fail(int *err) const {
    if (threadIdx.x == 0) atomicOr(err, 1);
    put(0.0);
  }
};
__device__ __forceinline__ FoldinCell foldin_cell(const FoldinArgs &a) {
  FoldinCell c;
  c.u = a.u0 + blockIdx.x;
  c.sl = blockIdx.y;
  c.s = a.s0 + c.sl;
  c.off = a.lin;
  c.M = a.K + c.off;
  c.w = a.wv[c.s];
  c.V = c.w + a.D;
  c.mu = a.mu + (size_t)c.s * (a.K + 1) + (1 - c.off);
  c.lam = a.lam + (size_t)c.s * (a.K + 1) + (1 - c.off);
  c.w0 = a.w0[c.s];
  c.e0 = a.eoff[c.u];
  c.e1 = a.eoff[c.u + 1];
  c.ow = a.out_w + (size_t)c.sl * gridDim.x + blockIdx.x;
  c.oV = a.out_V + ((size_t)c.sl * gridDim.x + blockIdx.x) * a.K;
  c.srow = (int64_t)c.s * a.U + c.u;
  return c;
}

// component j of the normals of (draw word, stream row): the Box-Muller value of counter word j >> 1, r cos for even j, r sin for odd j
__device__ __forceinline__ double foldin_normal(uint64_t seed, uint64_t word, int64_t srow, int j) {
  RowRng g(seed ^ ((uint64_t)(srow >> 32) * 0x9E3779B97F4A7C15ull), word, (uint32_t)srow);
  g.n = (uint32_t)(j >> 1);
  const double2 un = g.next2();
  const double r = sqrt(-2.0 * log(un.x));
  double sn, cs;
  sincospi(2.0 * un.y, &sn, &cs);
  return (j & 1) ? r * sn : r * cs;
}

// A = 0 and the (i, j) table of its upper triangle; the caller's barrier follows
__device__ __forceinline__ void foldin_gram_zero(double *A, uint16_t *tab, int M) {
  for (int t = threadIdx.x; t < M * M; t += FOLDIN_WG) {
    const int i = t / M, j = t - i * M;
    A[t] = 0.0;
    if (i <= j) tab[i * M - (i * (i - 1)) / 2 + (j - i)] = (uint16_t)(i | (j << 8));
  }
}
// entry e < T of the upper triangle takes the pass's share of sum z z^T, row after row (thread e of every FOLDIN_WG owns it)
__device__ __forceinline__ void foldin_gram_add(double *A, const uint16_t *tab, const double *Z, int M, int e, int nr) {
  const int ldz = M | 1, ij = tab[e], i = ij & 255, j = ij >> 8;
  double acc = A[i * M + j];
  for (int r = 0; r < nr; r++) acc = fma(Z[r * ldz + i], Z[r * ldz + j], acc);
  A[i * M + j] = acc;
}

// Lambda = U^T U in place (right-looking; every entry takes its updates in column order). True when a pivot is not positive and
// finite: every thread reads the same value, so the exit is uniform.
__device__ __forceinline__ bool foldin_factor(double *A, int M) {
  const int tid = threadIdx.x;
  for (int j = 0; j < M; j++) {
    const double d = A[j * M + j];
    if (!(d > 0.0) || !(d < INFINITY)) return true;
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
  return false;
}

// value (row r, component k) of the kept operand from the workgroup's LDS: W below the diagonal where the inversion left it (the
// lower triangle of A), its diagonal in dinv, theta_mean in bv
__device__ __forceinline__ void foldin_keep_write(double *__restrict__ Wf, int M, const double *A, const double *dinv, const double *bv) {
  const int KS4 = foldin_keep_ksteps(M), n = (int)foldin_keep_doubles(M);
  for (int e = threadIdx.x; e < n; e += FOLDIN_WG) {
    const int tq = e >> 6, t = tq / KS4, q = tq - t * KS4;
    const int r = t * 16 + (e & 15), k = q * 4 + ((e >> 4) & 3);
    double v = 0.0;
    if (k < M) {
      if (r < M)
        v = k < r ? A[r * M + k] : k == r ? dinv[r] : 0.0;
      else if (r == M)
        v = bv[k];
    }
    Wf[e] = v;
  }
}

// KEEP (mfm_foldin_rank.hpp): after the solves the triangular factor is inverted in LDS and written with the mean
// as the left operand of the ranking contraction (a.Wf); the means themselves are still written. KEEP excludes DRAW.
template <bool DRAW, bool KEEP = false>
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin(FoldinArgs a) {
  static_assert(!(DRAW && KEEP), "the kept operand holds the posterior mean");
  extern __shared__ double foldin_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FoldinCell c = foldin_cell(a);
  const int off = c.off, M = c.M, ldz = M | 1;
  const int T = M * (M + 1) / 2;
  const auto [A, bv, res, Z, part, tab] = foldin_lds(foldin_smem, M);
  const double *mu = c.mu, *lam = c.lam;
  const double alpha = a.alpha[c.s];
  double *Wf = KEEP ? a.Wf + ((size_t)blockIdx.x * a.S_all + c.s) * foldin_keep_doubles(M) : nullptr;
  const double eps = DRAW && tid < M ? foldin_normal(a.seed, FOLDIN_DRAW_TAG, c.srow, tid) : 0.0;

  if (c.e1 == c.e0) {  // no rows: the prior itself, mu bit for bit (the factorisation would round lambda mu / sqrt(lambda) / sqrt(lambda))
    double t = 0.0;
    if (tid < M) {
      t = mu[tid];
      if (DRAW) t = t + eps / sqrt(lam[tid]);
    }
    c.put(t);
    if constexpr (KEEP) {  // the prior: W = diag(1 / sqrt(lambda)), theta_mean = mu
      for (int t = tid; t < M * M; t += FOLDIN_WG) A[t] = 0.0;
      if (tid < M) {
        Z[tid] = 1.0 / sqrt(lam[tid]);
        bv[tid] = mu[tid];
      }
      __syncthreads();
      foldin_keep_write(Wf, M, A, Z, bv);
    }
    return;
  }

  foldin_gram_zero(A, tab, M);
  for (int t = tid; t < M; t += FOLDIN_WG) bv[t] = 0.0;
  __syncthreads();

  for (int64_t rb = c.e0; rb < c.e1; rb += FOLDIN_ROWS) {
    const int nr = (int)(c.e1 - rb < FOLDIN_ROWS ? c.e1 - rb : FOLDIN_ROWS);
    // ---- z, f and the residual of rows [rb, rb + nr)
    {
      const FoldinDD f = foldin_rows_zf(a, c.w, c.V, c.w0, rb, nr, Z, part);
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
        foldin_gram_add(A, tab, Z, M, e, nr);
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

  if (foldin_factor(A, M)) {  // a non-finite or non-positive lambda
    c.fail(a.err);
    if constexpr (KEEP)
      for (int e = tid; e < (int)foldin_keep_doubles(M); e += FOLDIN_WG) Wf[e] = 0.0;
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
  c.put(tid < M ? bv[tid] : 0.0);

  if constexpr (KEEP) {
    // ---- X = U^-1 column by column, thread r column r by back substitution: X[i][r] = -(sum_{i < j <= r} U[i][j] X[j][r]) / U[i][i]
    // from X[r][r] = 1 / U[r][r]. W = X^T: W[r][i] goes to A[r][i] below the diagonal, which the factorisation never touched, the
    // diagonal to Z (the passes are over); a thread reads the upper triangle and its own row only.
    __syncthreads();
    if (tid < M) {
      const int r = tid;
      const double xr = 1.0 / A[r * M + r];
      Z[r] = xr;
      for (int i = r - 1; i >= 0; i--) {
        double acc = A[i * M + r] * xr;
        for (int j = i + 1; j < r; j++) acc = fma(A[i * M + j], A[r * M + j], acc);
        A[r * M + i] = -acc / A[i * M + i];
      }
    }
    __syncthreads();
    foldin_keep_write(Wf, M, A, Z, bv);
  }
}

}  // namespace mfm
