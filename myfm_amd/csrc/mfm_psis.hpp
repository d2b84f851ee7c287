// mfm_psis.hpp -- Pareto-smoothed importance-sampling leave-one-out over the kept samples (not in the reference):
// per row of the design, with l_s = log p(y | theta_s) (logdens_value, mfm_logdens.hpp) and the importance ratios r_s = -l_s - max(-l),
// the largest M ratios are replaced by the quantiles of a generalized Pareto distribution fitted to them (Zhang and Stephens 2009
// with the loo package's priors: Vehtari, Gelman and Gabry 2017, Vehtari et al. 2024), the log weights are normalised, and
// elpd_loo = logsumexp_s(lw_s + l_s), the fit's shape k^ as the diagnostic, lpd as k_row_logdens computes it and for regression
// loo_pit = sum_s exp(lw_s) Phi(z_s) are written. Included by mfm_hip.hip after mfm_logdens.hpp.
//
// The tiled pass is that of mfm_dist.hpp (dist_tiles_run: the scores of a row tile, sample-major, in the scratch); its stage 2
// here, k_row_psis, follows the LDS form of k_row_summary. Everything is fp64, there are no atomics; every sum over samples runs
// in sample order and the sums over the grid in grid order, so a row's result depends on its own samples alone: another row tile,
// sample chunk, number of rows per workgroup or a rerun give the same bits. mfm_psis_row runs one row on the host through the
// same scalar pieces in the same orders.
#pragma once
#include <algorithm>
#include <numeric>

namespace mfm {

constexpr int PSIS_MIN_TAIL = 5;     // a shorter tail is not fitted (S <= 20 at r_eff = 1: ceil(0.2 S) < 5)
constexpr int PSIS_MAX_ROWS = 32;    // rows per workgroup
constexpr int PSIS_LDS_BYTES = 64 * 1024;       // per workgroup, where more than one row fits
constexpr int PSIS_LDS_MAX_BYTES = 160 * 1024;  // what a workgroup of gfx950 can have: one row of DIST_MAX_S samples takes 114 744 B

// ---- the scalar pieces, host and device ----------------------------------------------------------------------------------------
// m = 30 + floor(sqrt M) grid points (M <= 820 for S <= 4096: m <= 58, a grid point per lane)
__host__ __device__ __forceinline__ int psis_grid_size(int M) { return 30 + (int)sqrt((double)M); }
// the tail's first quartile x* sits at this index of the ascending tail
__host__ __device__ __forceinline__ int psis_quartile_index(int M) { return (int)floor((double)M / 4.0 + 0.5) - 1; }
// no fit: the tail is too short, or its lower quarter equals the cutoff (x* = exp(r) - exp(c) <= 0)
__host__ __device__ __forceinline__ bool psis_tail_too_short(int M) { return M < PSIS_MIN_TAIL; }
__host__ __device__ __forceinline__ bool psis_tail_degenerate(double x_star) { return x_star <= 0.0; }
// grid point j = 1 .. m
__host__ __device__ __forceinline__ double psis_grid_b(int j, int m, double x_max, double x_star) {
  return 1.0 / x_max + (1.0 - sqrt((double)m / ((double)j - 0.5))) / (3.0 * x_star);
}
// mean_i log1p(-b x_i) over the ascending tail, summed in that order
__host__ __device__ __forceinline__ double psis_profile_k(double b, const double *x, int M) {
  double sum = 0.0;
  for (int i = 0; i < M; i++) sum += log1p(-b * x[i]);
  return sum / (double)M;
}
// a grid point's k_j and profile log likelihood L_j
__host__ __device__ __forceinline__ void psis_grid_point(double b, const double *x, int M, double &k, double &L) {
  k = psis_profile_k(b, x, M);
  L = (double)M * (log(-b / k) - k - 1.0);
}
// k^ from the fitted k: the weakly informative prior of the loo package, worth 10 observations at 0.5
__host__ __device__ __forceinline__ double psis_khat(double k, int M) { return ((double)M * k + 5.0) / ((double)M + 10.0); }
// the smoothed value of tail element i (ascending): min(0, log(exp(c) + the GPD quantile at p_i = (i + 0.5) / M))
__host__ __device__ __forceinline__ double psis_smoothed(int i, int M, double khat, double sigma, double c_e) {
  const double p = ((double)i + 0.5) / (double)M;
  const double l1 = log1p(-p);
  const double q = khat == 0.0 ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
  return fmin(0.0, log(c_e + q));
}
// (value, sample index) pairs in ascending order, ties by sample index
__host__ __device__ __forceinline__ bool psis_after(double x0, int i0, double x1, int i1) { return x0 > x1 || (x0 == x1 && i0 > i1); }

struct RowPsisArgs {
  double *scratch;    // [S][Tn] the tile's scores; KEEP_W: the normalised log weights in their place on exit
  const double *y;    // of the tile's first row
  const double *aux;  // the per-sample constants of k_row_logdens
  double *lpd, *elpd, *khat, *pit;  // of the tile's first row (pit: regression only)
  int64_t Tn;
  int S, n_cut;
  int aux_lds;        // the constants are staged in LDS behind the rows
  int M, m, q;        // the tail's length (< PSIS_MIN_TAIL: no fit and no sort), the grid's size, the index of x* in the tail
  int P, R;           // S padded to a power of two (0 without a fit), rows per workgroup
  int st, stv;        // doubles per row of l and w (S | 1) and of the sort buffer (max(S, P) | 1): odd, the row-per-lane phases are conflict-free
  double log_S;
};

// LDS, in doubles: hdr[R][4] (min l or a flag, k^, a maximum, a log-sum-exp), l[R][st], w[R][st], v[R][stv], the sample indices
// idx[R][P] (ints), the per-sample constants where they are staged
static size_t psis_lds_doubles(int R, int st, int stv, int P, size_t n_aux) {
  return (size_t)R * (4 + 2 * (size_t)st + (size_t)stv + (size_t)P / 2) + n_aux;
}

// Stage 2, one launch per row tile. A workgroup brings R rows into LDS, every score turned into l on its way (all threads); lane r
// then walks row r in sample order for lpd (the recurrence of k_row_logdens) and min l. The ratios r_s = min l - l_s go into w (by
// sample) and with their sample index into the sort buffer, which one bitonic network over P = S padded with +inf orders for all R
// rows. A wavefront then fits a row: its lanes turn the tail into x_i in place, lane j walks them for grid point j (one LDS address
// for all lanes: a broadcast), the weights and b^ are summed over the lanes in grid order by shuffles, and lanes i < M write the
// smoothed values into w by sample index. The normalisation takes its exponentials with all threads and adds them up in sample
// order, a row per lane. Regression reads the score again from the scratch (L2) for Phi(z). Rows with an l of -inf leave with
// elpd = -inf, k^ = +inf and NaN weights.
template <int TASK, bool KEEP_W>
__global__ __launch_bounds__(WG) void k_row_psis(RowPsisArgs a) {
  extern __shared__ double psis_lds[];
  const int S = a.S, R = a.R, st = a.st, stv = a.stv, P = a.P, M = a.M, n_cut = a.n_cut;
  double *hdr = psis_lds, *l = hdr + 4 * R, *w = l + (size_t)R * st, *v = w + (size_t)R * st;
  int *idx = reinterpret_cast<int *>(v + (size_t)R * stv);
  double *staged = v + (size_t)R * stv + (size_t)R * (P / 2);
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(a.Tn - r0 < R ? a.Tn - r0 : R);
  const int tid = threadIdx.x;
  const bool use_staged = TASK != LOGDENS_CLASSIFICATION && a.aux_lds;
  if (use_staged) {
    const int n_aux = TASK == LOGDENS_REGRESSION ? 2 * S : S * n_cut;
    for (int i = tid; i < n_aux; i += WG) staged[i] = a.aux[i];
    __syncthreads();
  }
  // (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto fill = [&](const double *aux) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      double lv = 0.0;
      if (r < nr) {
        const double score = a.scratch[(size_t)s * a.Tn + r0 + r], yt = a.y[r0 + r];
        if constexpr (TASK == LOGDENS_REGRESSION)
          lv = logdens_value<TASK>(yt, score, aux[s], aux[S + s], nullptr, 0);
        else if constexpr (TASK == LOGDENS_CLASSIFICATION)
          lv = logdens_value<TASK>(yt, score, 0.0, 0.0, nullptr, 0);
        else
          lv = logdens_value<TASK>(yt, score, 0.0, 0.0, aux + (size_t)s * n_cut, n_cut);
      }
      l[r * st + s] = lv;
    }
  };
  if (use_staged)
    fill(staged);
  else
    fill(a.aux);
  __syncthreads();
  if (tid < nr) {
    const double *row = l + tid * st;
    double m = 0.0, acc = 0.0, lmin = row[0];
    for (int s = 0; s < S; s++) {
      const double lv = row[s];
      MFM_LOGDENS_LSE_STEP(s, lv, m, acc)
      lmin = fmin(lmin, lv);
    }
    a.lpd[r0 + tid] = m + log(acc) - a.log_S;
    hdr[4 * tid] = lmin;  // (-inf: the row has a density of 0 under some sample)
    hdr[4 * tid + 1] = __builtin_inf();
  }
  __syncthreads();
  for (int i = tid; i < S * R; i += WG) {
    const int s = i / R, r = i - s * R;
    const double lmin = r < nr ? hdr[4 * r] : 0.0;
    const double rv = lmin == -__builtin_inf() ? 0.0 : lmin - l[r * st + s];  // = -l - max(-l)
    w[r * st + s] = rv;
    if (P) {
      v[r * stv + s] = rv;
      idx[r * P + s] = s;
    }
  }
  for (int i = tid; i < (P - S) * R; i += WG) {  // (P = 0: no iteration)
    const int s = S + i / R, r = i % R;
    v[r * stv + s] = __builtin_inf();
    idx[r * P + s] = s;
  }
  __syncthreads();
  if (P) {
    const int half = P >> 1;
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int e = tid; e < R * half; e += WG) {
          const int r = e / half, c2 = e - r * half;
          const int i = ((c2 & ~(j - 1)) << 1) | (c2 & (j - 1));
          double *vr = v + r * stv;
          int *ir = idx + r * P;
          const double x0 = vr[i], x1 = vr[i | j];
          const int i0 = ir[i], i1 = ir[i | j];
          if (psis_after(x0, i0, x1, i1) == ((i & k) == 0)) {
            vr[i] = x1;
            vr[i | j] = x0;
            ir[i] = i1;
            ir[i | j] = i0;
          }
        }
        __syncthreads();
      }
    // the fit, a row per wavefront (every wavefront makes the same number of rounds: the barriers are uniform)
    const int lane = tid & (WAVE - 1), wave = tid / WAVE;
    for (int rb = 0; rb < R; rb += WG / WAVE) {
      const int r = rb + wave;
      const bool on = r < nr && hdr[4 * (r < nr ? r : 0)] != -__builtin_inf();
      double *tail = v + (r < R ? r : 0) * stv + (S - M);  // ascending; M < S (the launcher)
      double c_e = 0.0;
      if (on) {
        c_e = exp(tail[-1]);  // the cutoff, position S - M - 1
        for (int i = lane; i < M; i += WAVE) tail[i] = exp(tail[i]) - c_e;
      }
      __syncthreads();
      if (on) {
        const double x_star = tail[a.q];
        if (!psis_tail_degenerate(x_star)) {  // (one value for the wavefront)
          const int m = a.m;
          const double b = psis_grid_b((lane < m ? lane : m - 1) + 1, m, tail[M - 1], x_star);
          double kj, Lj;
          psis_grid_point(b, tail, M, kj, Lj);
          double den = 0.0;
          for (int i = 0; i < m; i++) den += exp(__shfl(Lj, i) - Lj);
          const double bw = b * (1.0 / den);
          double bhat = 0.0;
          for (int j = 0; j < m; j++) bhat += __shfl(bw, j);
          const double k = psis_profile_k(bhat, tail, M), sigma = -k / bhat, khat = psis_khat(k, M);
          const int *ti = idx + r * P + (S - M);
          for (int i = lane; i < M; i += WAVE) {
            const int si = ti[i];  // (a padding index can stand here only if a ratio was NaN: scores are finite)
            if (si < S) w[r * st + si] = psis_smoothed(i, M, khat, sigma, c_e);
          }
          if (lane == 0) hdr[4 * r + 1] = khat;
        }
      }
    }
    __syncthreads();
  }
  // lw_s = w_s - logsumexp_s w_s: the maximum (a row per lane), the exponentials (all threads), their sum in sample order
  if (tid < nr) {
    const double *row = w + tid * st;
    double mx = row[0];
    for (int s = 1; s < S; s++) mx = fmax(mx, row[s]);
    hdr[4 * tid + 2] = mx;
  }
  __syncthreads();
  for (int i = tid; i < S * R; i += WG) {
    const int s = i / R, r = i - s * R;
    v[r * stv + s] = r < nr ? exp(w[r * st + s] - hdr[4 * r + 2]) : 0.0;
  }
  __syncthreads();
  if (tid < nr) {
    const double *row = v + tid * stv, *wr = w + tid * st, *lr = l + tid * st;
    double sum = 0.0;
    for (int s = 0; s < S; s++) sum += row[s];
    const double lse = hdr[4 * tid + 2] + log(sum);
    double mx = (wr[0] - lse) + lr[0];
    for (int s = 1; s < S; s++) mx = fmax(mx, (wr[s] - lse) + lr[s]);
    hdr[4 * tid + 3] = lse;
    hdr[4 * tid + 2] = mx;
  }
  __syncthreads();
  // elpd_loo = logsumexp_s(lw_s + l_s), loo_pit = sum_s exp(lw_s) Phi(z_s): the terms with all threads (the pit's in l's place)
  const auto terms = [&](const double *aux) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      if (r >= nr) continue;
      const bool zero = hdr[4 * r] == -__builtin_inf();
      const double lw = w[r * st + s] - hdr[4 * r + 3], lv = zero ? 0.0 : l[r * st + s];
      v[r * stv + s] = exp((lw + lv) - hdr[4 * r + 2]);
      if constexpr (TASK == LOGDENS_REGRESSION) {
        const double score = a.scratch[(size_t)s * a.Tn + r0 + r];
        l[r * st + s] = exp(lw) * (0.5 * erfc(-((a.y[r0 + r] - score) * aux[S + s]) * 0.70710678118654752440));
      }
      if (KEEP_W) a.scratch[(size_t)s * a.Tn + r0 + r] = zero ? __builtin_nan("") : lw;
    }
  };
  if (use_staged)
    terms(staged);
  else
    terms(a.aux);
  __syncthreads();
  if (tid < nr) {
    const double *row = v + tid * stv, *pr = l + tid * st;
    const bool zero = hdr[4 * tid] == -__builtin_inf();
    double sum = 0.0, pit = 0.0;
    for (int s = 0; s < S; s++) sum += row[s];
    a.elpd[r0 + tid] = zero ? -__builtin_inf() : hdr[4 * tid + 2] + log(sum);
    a.khat[r0 + tid] = zero ? __builtin_inf() : hdr[4 * tid + 1];
    if constexpr (TASK == LOGDENS_REGRESSION) {
      for (int s = 0; s < S; s++) pit += pr[s];
      a.pit[r0 + tid] = zero ? __builtin_nan("") : pit;
    }
  }
}

template <int TASK, bool KEEP_W>
static void launch_row_psis_form(hipStream_t s, const RowPsisArgs &a, size_t lds) {
  static DeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {  // above the default limit of dynamic LDS (opted into once per device)
    void (*const kernel)(RowPsisArgs) = k_row_psis<TASK, KEEP_W>;
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PSIS_LDS_MAX_BYTES));
    raised.mark();
  }
  hipLaunchKernelGGL((k_row_psis<TASK, KEEP_W>), dim3((unsigned)cdiv(a.Tn, a.R)), dim3(WG), lds, s, a);
}
// n_aux: the per-sample constants, in doubles. Sized next to launch_row_summary's arithmetic (mfm_dist.hpp): R rows of
// 4 + 2 (S | 1) + (max(S, P) | 1) + P / 2 doubles within PSIS_LDS_BYTES, at most PSIS_MAX_ROWS and never less than one row
// (S = 4096: 14 343 doubles = 114 744 B, R = 1); the constants behind them where the budget still holds them.
static void launch_row_psis(hipStream_t s, int task, RowPsisArgs &a, size_t n_aux, bool keep_w) {
  int P = 0;
  if (!psis_tail_too_short(a.M)) {
    P = 1;
    while (P < a.S) P <<= 1;  // (M >= 5 of at most 0.2 S: P >= 32)
  }
  a.P = P;
  a.st = a.S | 1;
  a.stv = std::max(a.S, P) | 1;
  a.m = psis_grid_size(a.M);
  a.q = psis_quartile_index(a.M);
  const size_t row = psis_lds_doubles(1, a.st, a.stv, P, 0);
  const size_t budget = PSIS_LDS_BYTES / sizeof(double);
  a.R = (int)std::min<int64_t>(std::max<int64_t>(1, std::min<int64_t>(PSIS_MAX_ROWS, (int64_t)(budget / row))), a.Tn);
  const size_t rows = psis_lds_doubles(a.R, a.st, a.stv, P, 0);
  a.aux_lds = n_aux > 0 && rows + n_aux <= budget;
  const size_t lds = (rows + (a.aux_lds ? n_aux : 0)) * sizeof(double);
  logdens_with_task(task, [&](auto task_c) {
    constexpr int T = decltype(task_c)::value;
    if (keep_w)
      launch_row_psis_form<T, true>(s, a, lds);
    else
      launch_row_psis_form<T, false>(s, a, lds);
  });
}

// One row on the host, sequentially, through the scalar pieces and in the summation orders of k_row_psis. out_lw[S] may be null.
static void psis_row_host(int S, int M, const double *ll, double *out_elpd, double *out_k, double *out_lw) {
  const double inf = std::numeric_limits<double>::infinity();
  double lmin = ll[0];
  for (int s = 0; s < S; s++) lmin = fmin(lmin, ll[s]);
  if (lmin == -inf) {
    *out_elpd = -inf;
    *out_k = inf;
    if (out_lw) std::fill(out_lw, out_lw + S, std::numeric_limits<double>::quiet_NaN());
    return;
  }
  std::vector<double> w((size_t)S);
  for (int s = 0; s < S; s++) w[(size_t)s] = lmin - ll[s];
  double khat = inf;
  if (!psis_tail_too_short(M)) {
    std::vector<int> idx((size_t)S);
    std::iota(idx.begin(), idx.end(), 0);
    std::sort(idx.begin(), idx.end(), [&](int i0, int i1) { return psis_after(w[(size_t)i1], i1, w[(size_t)i0], i0); });
    const double c_e = exp(w[(size_t)idx[(size_t)(S - M - 1)]]);
    std::vector<double> x((size_t)M);
    for (int i = 0; i < M; i++) x[(size_t)i] = exp(w[(size_t)idx[(size_t)(S - M + i)]]) - c_e;
    const double x_star = x[(size_t)psis_quartile_index(M)];
    if (!psis_tail_degenerate(x_star)) {
      const int m = psis_grid_size(M);
      std::vector<double> b((size_t)m), L((size_t)m);
      for (int j = 0; j < m; j++) {
        double kj;
        b[(size_t)j] = psis_grid_b(j + 1, m, x[(size_t)(M - 1)], x_star);
        psis_grid_point(b[(size_t)j], x.data(), M, kj, L[(size_t)j]);
      }
      double bhat = 0.0;
      for (int j = 0; j < m; j++) {
        double den = 0.0;
        for (int i = 0; i < m; i++) den += exp(L[(size_t)i] - L[(size_t)j]);
        bhat += b[(size_t)j] * (1.0 / den);
      }
      const double k = psis_profile_k(bhat, x.data(), M), sigma = -k / bhat;
      khat = psis_khat(k, M);
      for (int i = 0; i < M; i++) w[(size_t)idx[(size_t)(S - M + i)]] = psis_smoothed(i, M, khat, sigma, c_e);
    }
  }
  double mx = w[0], sum = 0.0;
  for (int s = 1; s < S; s++) mx = fmax(mx, w[(size_t)s]);
  for (int s = 0; s < S; s++) sum += exp(w[(size_t)s] - mx);
  const double lse = mx + log(sum);
  double amax = (w[0] - lse) + ll[0];
  for (int s = 1; s < S; s++) amax = fmax(amax, (w[(size_t)s] - lse) + ll[s]);
  sum = 0.0;
  for (int s = 0; s < S; s++) {
    const double lw = w[(size_t)s] - lse;
    sum += exp((lw + ll[s]) - amax);
    if (out_lw) out_lw[s] = lw;
  }
  *out_elpd = amax + log(sum);
  *out_k = khat;
}

// The checks of a leave-one-out call on top of logdens_check; nothing here touches the device. The call is a LogdensCall whose
// out_mean / out_var / out_ll are elpd_loo, k^ and the log weights.
static void loo_check(const LogdensCall &c, int64_t N, int count, int32_t tail_len) {
  logdens_check(c, N, count);
  if (count > DIST_MAX_S)
    throw Error(MFM_ERR_INVALID, "leave-one-out weights are computed over at most " + std::to_string(DIST_MAX_S) + " samples, got " + std::to_string(count));
  if (tail_len < 0 || (count > 0 && tail_len >= count)) throw Error(MFM_ERR_INVALID, "tail_len must lie in [0, S)");
  if (psis_grid_size(tail_len) > WAVE)  // (never for tail_len <= 0.2 S: 30 + floor(sqrt 819) = 58)
    throw Error(MFM_ERR_INVALID, "tail_len above 1155: its grid of 30 + floor(sqrt(tail_len)) points must fit one wavefront");
}

static void design_loo(mfm_design *d, const SampleView &v, const LogdensCall &c, int32_t tail_len) {
  const int count = v.count();
  check_sample_source(d, v);
  hipStream_t s = d->stream;
  const size_t N = (size_t)d->N;
  if (N == 0) return;
  const bool pit = c.task == LOGDENS_REGRESSION;
  const int64_t T = dist_tiles_reserve(d, v, c.tile_rows, N * 4);  // lpd, elpd, k, pit
  const LogdensConstants k = logdens_upload(d, s, c, d->N, count);
  RowPsisArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scratch = d->dist_scratch.p;
  a.aux = k.aux;
  a.S = count;
  a.n_cut = c.task == LOGDENS_ORDERED ? c.n_cut : 0;
  a.M = tail_len;
  a.log_S = std::log((double)count);
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    a.Tn = Tn;
    a.y = d->dist_y.p + r0;
    a.lpd = d->dist_out.p + r0;
    a.elpd = d->dist_out.p + N + r0;
    a.khat = d->dist_out.p + 2 * N + r0;
    a.pit = pit ? d->dist_out.p + 3 * N + r0 : nullptr;
    launch_row_psis(s, c.task, a, k.n_aux, c.out_ll != nullptr);
  };
  // out_ll: the tile's log weights, which KEEP_W leaves in the scratch; the call's out_mean / out_var are elpd_loo / k^ (loo_check)
  dist_tiles_run(d, v, T, 0, c.chunk_samples, c.out_ll,
                 {{c.out_lpd, 0, N}, {c.out_mean, N, N}, {c.out_var, 2 * N, N}, {c.out_pit, 3 * N, pit && c.out_pit ? N : 0}}, stage2);
}

}  // namespace mfm

extern "C" {

int mfm_design_loo_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y, const double *precisions,
                         int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples, int32_t tail_len, double *out_elpd,
                         double *out_k, double *out_lpd, double *out_pit, double *out_lw) {
  MFM_TRY(d)
  const LogdensCall c{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_lpd, out_elpd, out_k, out_pit, out_lw};
  loo_check(c, d->N, std::max(count, 0), tail_len);
  design_loo(d, samples_of_store(st, first, count), c, tail_len);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_loo(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t task,
                   const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                   int32_t tail_len, double *out_elpd, double *out_k, double *out_lpd, double *out_pit, double *out_lw) {
  MFM_TRY(d)
  const LogdensCall c{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_lpd, out_elpd, out_k, out_pit, out_lw};
  loo_check(c, d->N, std::max(n_samples, 0), tail_len);
  store_check_fraction(d->D, rank, n_samples);
  design_loo(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), c, tail_len);
  MFM_CATCH(d)
}

// one row of k_row_psis on the host, by the scalar pieces the kernel runs (no device): log_lik[S], tail_len in [0, S)
int mfm_psis_row(int32_t S, int32_t tail_len, const double *log_lik, double *out_elpd, double *out_k, double *out_lw) {
  if (S < 1 || S > mfm::DIST_MAX_S || tail_len < 0 || tail_len >= S || !log_lik || !out_elpd || !out_k) {
    g_global_error = "a row of 1 to " + std::to_string(mfm::DIST_MAX_S) + " log likelihoods, tail_len in [0, S) and the two outputs are needed";
    return MFM_ERR_INVALID;
  }
  try {
    mfm::psis_row_host(S, tail_len, log_lik, out_elpd, out_k, out_lw);
  } catch (const std::bad_alloc &) {
    g_global_error = "host out of memory";
    return MFM_ERR_RUNTIME;
  }
  return MFM_OK;
}

}  // extern "C"
