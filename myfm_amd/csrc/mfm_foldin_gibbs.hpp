// mfm_foldin_gibbs.hpp -- the kernel of mfm_foldin_gibbs_* (mfm_foldin_gibbs.hip): the parameters of a NEW one-hot
// feature u under one kept sample of a probit model (classifier or ordered probit), by a short Albert-Chib chain on chip. As in
// mfm_foldin.hpp the feature enters the score linearly, score_s(x + e_u) = f_s(x) + z(x)^T theta with z = (1, q_s(x)); both probit
// tasks have noise precision 1, so Lambda = diag(lambda) + sum_i z_i z_i^T is fixed for the whole chain. From theta^0 = mu, sweep t:
//   m_i = f_i + z_i^T theta^t,   d_i = the truncated standard normal of row i's label around -m_i (the cutpoints minus m_i),
//   r_i = z_i^T theta^t + d_i,   b = lambda mu + sum_i z_i r_i,   thetabar^{t+1} = Lambda^-1 b,   theta^{t+1} = thetabar^{t+1} + U^-1 eps^t.
// One workgroup owns one (entity, sample). The setup pass is mfm_foldin.hpp's (foldin_rows_zf); it also keeps every row's z
// (transposed, [M][n_u]: a sweep's row-parallel reads coalesce) and f (rounded to one double: it enters a truncation bound, not a
// residual) in the cell's device scratch. Lambda = U^T U is factored once and W = U^-1 formed in place, its transpose mirrored into
// the unused lower triangle: a sweep's y = W^T b and (thetabar, theta) = W (y, y + eps) are then column walks of one LDS matrix
// with two barriers, instead of 2 M barrier-separated substitution steps per sweep.
// A sweep walks the rows in passes of FOLDIN_WG, one thread per row (dot product with theta from LDS, the draw, r_i to LDS); then
// sum_i z_i r_i is accumulated by fixed owners: thread (j, g), g < NG = FOLDIN_WG / M, adds rows g, g + NG, .. of every pass to its
// partial of component j in row order, and component j's thread adds the NG partials in g order. No order depends on the grid, the
// chunking or the scratch bound.
#pragma once
#include "mfm_foldin.hpp"
#include "mfm_foldin_gibbs_plan.hpp"
#include "mfm_tn.hpp"

namespace mfm {

// draw words of the per-row Philox streams. Latent draw of grouped row i at sweep t: (seed, FOLDIN_LATENT_TAG + t, row = s n + i),
// the counter words being the attempts of the rejection loop. eps^t_j: (seed, FOLDIN_DRAW_TAG + 1 + t, row = s U + u), component j
// the Box-Muller value of counter word j >> 1 as in k_foldin<true>, whose own word FOLDIN_DRAW_TAG stays untouched.
constexpr uint64_t FOLDIN_LATENT_TAG = 0x464F4C444C540000ull;  // "FOLDLT" << 16: t <= 65535 fits below

struct FoldinGibbsArgs {
  FoldinArgs a;       // (alpha is not read; y holds the labels: +-1, or class indices)
  const double *cut;  // [S][n_class - 1], ordered probit
  int n_class, n_burn, n_inner;
  int64_t n;          // the handle's row count (the latent stream's row is s n + i)
  double *zf;         // [gridDim.y][rows][M + 1]: per sample of the launch the cells of its entities, z^T then f each
  int64_t rows;       // rows of the launch's entities, eoff[u0 + gridDim.x] - eoff[u0]
};

// component j of the normals of (draw word, stream row)
__device__ __forceinline__ double foldin_normal(uint64_t seed, uint64_t word, int64_t srow, int j) {
  RowRng g(seed ^ ((uint64_t)(srow >> 32) * 0x9E3779B97F4A7C15ull), word, (uint32_t)srow);
  g.n = (uint32_t)(j >> 1);
  const double2 un = g.next2();
  const double r = sqrt(-2.0 * log(un.x));
  double sn, cs;
  sincospi(2.0 * un.y, &sn, &cs);
  return (j & 1) ? r * sn : r * cs;
}

template <int TASK, bool DRAW>
__global__ __launch_bounds__(FOLDIN_WG) void k_foldin_gibbs(FoldinGibbsArgs ga) {
  extern __shared__ double foldin_smem[];
  const FoldinArgs &a = ga.a;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, off = a.lin, M = K + off, ldz = M | 1;
  const int T = M * (M + 1) / 2;
  const int sweeps = ga.n_burn + ga.n_inner;
  double *A = foldin_smem;                    // [M][M]: the Gram sums, Lambda, U, then W = U^-1 (upper) and W^T (lower)
  double *bv = A + M * M;                     // [M]: b of the sweep
  double *Z = bv + M;                         // [FOLDIN_ROWS][ldz]: the setup pass's z
  double *res = Z + FOLDIN_ROWS * ldz;        // [FOLDIN_ROWS]: (the setup pass's flag of a non-finite f sits in its first word)
  double *part = res + FOLDIN_ROWS;           // [2][4][FOLDIN_ROWS]
  uint16_t *tab = (uint16_t *)(part + 2 * (FOLDIN_WG / 64) * FOLDIN_ROWS);  // [T]
  // the sweeps' arrays lie over Z, res and part (5 M + 2 FOLDIN_WG <= 64 ldz + 64 + 512 doubles), which the setup pass is done with
  double *theta = Z;                          // [M]
  double *yv = theta + M;                     // [M]: W^T b
  double *ye = yv + M;                        // [M]: W^T b + eps
  double *lmu = ye + M;                       // [M]: lambda mu
  double *rl = lmu + M;                       // [FOLDIN_WG]: the pass's r
  double *pb = rl + FOLDIN_WG;                // [FOLDIN_WG]: the owners' partial sums of z r

  const int64_t u = a.u0 + blockIdx.x;
  const int sl = blockIdx.y, s = a.s0 + sl;
  const double *__restrict__ w = a.wv[s];
  const double *__restrict__ V = w + a.D;
  const double *__restrict__ mu = a.mu + (size_t)s * (K + 1) + (1 - off);
  const double *__restrict__ lam = a.lam + (size_t)s * (K + 1) + (1 - off);
  const double w0 = a.w0[s];
  const int64_t e0 = a.eoff[u], e1 = a.eoff[u + 1], nu = e1 - e0;
  double *__restrict__ ow = a.out_w + (size_t)sl * gridDim.x + blockIdx.x;
  double *__restrict__ oV = a.out_V + ((size_t)sl * gridDim.x + blockIdx.x) * K;
  const int64_t srow = (int64_t)s * a.U + u;

  if (nu == 0) {  // no rows: the prior itself, mu bit for bit; a draw: the chain's last step from it
    if (tid < M) {
      double t = mu[tid];
      if (DRAW) t = t + foldin_normal(a.seed, FOLDIN_DRAW_TAG + (uint64_t)sweeps, srow, tid) / sqrt(lam[tid]);
      if (off && tid == 0)
        *ow = t;
      else
        oV[tid - off] = t;
    }
    if (!off && tid == 0) *ow = 0.0;
    return;
  }
  // the cell's scratch: z^T [M][nu], then f [nu]
  double *__restrict__ zT = ga.zf + ((size_t)sl * ga.rows + (size_t)(e0 - a.eoff[a.u0])) * (size_t)(M + 1);
  double *__restrict__ fS = zT + (size_t)M * nu;

  for (int t = tid; t < M * M; t += FOLDIN_WG) {
    const int i = t / M, j = t - i * M;
    A[t] = 0.0;
    if (i <= j) tab[i * M - (i * (i - 1)) / 2 + (j - i)] = (uint16_t)(i | (j << 8));
  }
  int *badf = (int *)res;
  if (tid == 0) *badf = 0;
  __syncthreads();

  // ---- the setup pass: z and f of every row into the scratch, sum z z^T (upper triangle) row after row
  for (int64_t rb = e0; rb < e1; rb += FOLDIN_ROWS) {
    const int nr = (int)(e1 - rb < FOLDIN_ROWS ? e1 - rb : FOLDIN_ROWS);
    const FoldinDD f = foldin_rows_zf(a, w, V, w0, rb, nr, Z, part);
    if (wave == 0) {
      if (lane < nr) {
        const double fv = f.hi + f.lo;
        fS[rb - e0 + lane] = fv;
        if (!(fabs(fv) < INFINITY)) *badf = 1;  // (a truncation bound that is not finite would only run the samplers dry)
      }
      if (off) Z[lane * ldz] = 1.0;
    }
    __syncthreads();
    for (int e = tid; e < M * nr; e += FOLDIN_WG) {
      const int j = e / nr, r = e - j * nr;
      zT[(size_t)j * nu + (size_t)(rb - e0) + r] = Z[r * ldz + j];
    }
    for (int e = tid; e < T; e += FOLDIN_WG) {
      const int ij = tab[e], i = ij & 255, j = ij >> 8;
      double acc = A[i * M + j];
      for (int r = 0; r < nr; r++) acc = fma(Z[r * ldz + i], Z[r * ldz + j], acc);
      A[i * M + j] = acc;
    }
    __syncthreads();
  }

  // ---- Lambda (noise precision 1)
  for (int e = tid; e < T; e += FOLDIN_WG) {
    const int ij = tab[e], i = ij & 255, j = ij >> 8;
    if (i == j) A[i * M + j] = lam[i] + A[i * M + j];
  }
  bool bad = *badf != 0;
  __syncthreads();

  // ---- Lambda = U^T U in place (right-looking; every entry takes its updates in column order)
  for (int j = 0; j < M && !bad; j++) {
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
  if (bad) {  // a non-finite model value or a non-positive pivot: reported through the handle, never a NaN in the result
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

  // ---- W = U^-1 in place, column after column: W[i][j] = -(sum_{i <= k < j} W[i][k] U[k][j]) / U[j][j], thread i row i
  for (int j = 0; j < M; j++) {
    const double d = A[j * M + j];
    double v = 1.0 / d;
    if (tid < j) {
      double acc = 0.0;
      for (int k = tid; k < j; k++) acc = fma(A[tid * M + k], A[k * M + j], acc);
      v = -acc / d;
    }
    __syncthreads();
    if (tid <= j) A[tid * M + j] = v;
    __syncthreads();
  }
  // W^T into the lower triangle, so that both of a sweep's products walk columns (thread i column i: no bank is hit twice)
  for (int t = tid; t < M * M; t += FOLDIN_WG) {
    const int i = t / M, k = t - i * M;
    if (k > i) A[k * M + i] = A[t];
  }
  if (tid < M) {
    theta[tid] = mu[tid];
    lmu[tid] = lam[tid] * mu[tid];
  }
  __syncthreads();

  // ---- the sweeps
  const int NG = FOLDIN_WG / M;  // owners per component
  const bool own = tid < M * NG;
  const int jo = tid / NG, go = tid - jo * NG;
  const double *__restrict__ zo = zT + (size_t)(own ? jo : 0) * nu;
  const double *__restrict__ gam = TASK == FOLDIN_TASK_ORDERED ? ga.cut + (size_t)s * (ga.n_class - 1) : nullptr;
  const int64_t lrow0 = (int64_t)s * ga.n + e0;
  double mean = 0.0;
  for (int t = 0; t < sweeps; t++) {
    double pacc = 0.0;
    for (int64_t p0 = 0; p0 < nu; p0 += FOLDIN_WG) {
      const int np = (int)(nu - p0 < FOLDIN_WG ? nu - p0 : FOLDIN_WG);
      if (tid < np) {
        const int64_t i = p0 + tid;
        double zt = 0.0;
        for (int j = 0; j < M; j++) zt = fma(zT[(size_t)j * nu + i], theta[j], zt);
        const double m = fS[i] + zt;
        const int64_t grow = lrow0 + i;
        RowRng g(a.seed ^ ((uint64_t)(grow >> 32) * 0x9E3779B97F4A7C15ull), FOLDIN_LATENT_TAG + (uint64_t)t, (uint32_t)grow);
        const double yl = a.y[e0 + i];
        double d;
        if (TASK == FOLDIN_TASK_CLASSIFIER) {
          d = yl > 0 ? tn_left(g, 0.0 - m) : tn_right(g, 0.0 - m);
        } else {
          const int cls = (int)yl;
          if (cls == 0)
            d = tn_right(g, gam[0] - m);
          else if (cls == ga.n_class - 1)
            d = tn_left(g, gam[ga.n_class - 2] - m);
          else
            d = tn_twoside(g, gam[cls - 1] - m, gam[cls] - m);
        }
        rl[tid] = zt + d;
      }
      __syncthreads();
      if (own)
        for (int r = go; r < np; r += NG) pacc = fma(zo[p0 + r], rl[r], pacc);
      __syncthreads();
    }
    if (own) pb[tid] = pacc;
    __syncthreads();
    if (tid < M) {
      double b = lmu[tid];
      for (int g = 0; g < NG; g++) b += pb[tid * NG + g];
      bv[tid] = b;
    }
    __syncthreads();
    if (tid < M) {  // y = W^T b: column tid of the upper triangle
      double y = 0.0;
      for (int k = 0; k <= tid; k++) y = fma(A[k * M + tid], bv[k], y);
      yv[tid] = y;
      ye[tid] = y + foldin_normal(a.seed, FOLDIN_DRAW_TAG + 1 + (uint64_t)t, srow, tid);
    }
    __syncthreads();
    if (tid < M) {  // W y and W (y + eps): column tid of the lower triangle
      double tb = 0.0, tt = 0.0;
      for (int k = tid; k < M; k++) {
        const double wk = A[k * M + tid];
        tb = fma(wk, yv[k], tb);
        tt = fma(wk, ye[k], tt);
      }
      theta[tid] = tt;
      if (t >= ga.n_burn) mean += tb;
    }
    __syncthreads();
  }
  if (tid < M) {
    const double v = DRAW ? theta[tid] : mean / (double)ga.n_inner;
    if (off && tid == 0)
      *ow = v;
    else
      oV[tid - off] = v;
  }
  if (!off && tid == 0) *ow = 0.0;
}

}  // namespace mfm
