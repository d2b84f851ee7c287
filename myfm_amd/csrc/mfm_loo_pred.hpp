// mfm_loo_pred.hpp -- leave-one-out predictions over the kept samples (not in the reference): the Pareto-smoothed
// importance weights w_s = exp(lw_s) of mfm_psis.hpp applied to what the samples predict. Per row of the design
//   summary   of the value v_s that predict_dist summarises (the score; Phi(score); the expected class index under the sample's
//             cutpoints): mean = sum_s w_s v_s, sd = sqrt(sum_s w_s (v_s - mean)^2), for regression sd_y = sqrt(sd^2 + sum_s w_s /
//             alpha_s), ess = 1 / sum_s w_s^2 and weighted quantiles by the inverse-CDF rule of the loo package's E_loo (below)
//   CRPS      of mfm_crps.hpp with the predictive distribution reweighted: regression accuracy = sum_s w_s A(y - mu_s, v_s),
//             p_s = sum_{u < s} w_u A(mu_s - mu_u, v_s + v_u) + w_s g(2 v_s) / 2, spread = sum_s w_s p_s, crps = accuracy - spread;
//             classification and ordered probit d_j = sum_s w_s Phi(+-t_sj), accuracy = sum_j d_j, spread = sum_j d_j (1 - d_j),
//             crps = sum_j d_j^2
// Included by mfm_hip.hip after mfm_psis.hpp and mfm_crps.hpp.
//
// The tiled pass is that of mfm_dist.hpp. Its stage 2 here runs in three steps on the design's stream: the tile's scores are copied
// device to device into d->loo_scores, k_row_psis<TASK, true> turns the scratch into the log weights (the kernel and the launch of
// predict_loo: k^ has its bits), k_loo_weights takes their exponential once per (row, sample), and the third stage -- k_row_loo_summary,
// k_row_loo_crps_mix or k_row_loo_crps_cdf -- reads both. Everything is fp64, there are no atomics, every sum runs in sample order
// (the pair sums in u order, then in s order; the cuts in cut order): a row's bits depend on its own samples alone. A row with an
// l_s of -inf has NaN weights: every output is NaN and k^ = +inf.
#pragma once

namespace mfm {

constexpr int LOO_CRPS_BLOCK = 4;  // samples whose pair sums a lane of k_row_loo_crps_mix holds in registers (the listing)

// ---- the scalar pieces, host and device ----------------------------------------------------------------------------------------
// The weighted quantile at probability p, reached at position i of the order by (value, sample): c_prev < p <= c, the running
// sums of the weights before and with position i. Position 0: the smallest value; else between the two neighbours.
__host__ __device__ __forceinline__ double loo_quantile_step(int i, double p, double v_prev, double v, double c_prev, double c) {
  if (i == 0) return v;
  const double f = (p - c_prev) / (c - c_prev);
  return v_prev + (v - v_prev) * fmin(1.0, fmax(0.0, f));
}
// One walk over the order for all n_q probabilities p[] (ascending): v(i), w(i) the value and the weight at position i;
// emit(q, x) takes quantile q. A probability that no running sum reaches (rounding, p near 1) gets the largest value.
template <class V, class W, class Emit>
__host__ __device__ __forceinline__ void loo_quantile_walk(int S, const V &v, const W &w, int n_q, const double *p, const Emit &emit) {
  int q = 0;
  double c = 0.0, v_prev = 0.0;
  for (int i = 0; i < S && q < n_q; i++) {
    const double vi = v(i), c_prev = c;
    c += w(i);
    while (q < n_q && c >= p[q]) {
      emit(q, loo_quantile_step(i, p[q], v_prev, vi, c_prev, c));
      q++;
    }
    v_prev = vi;
  }
  if (q < n_q) {
    const double last = v(S - 1);
    for (; q < n_q; q++) emit(q, last);
  }
}
// the weighted pair term and the weighted own term of a regression CRPS
__host__ __device__ __forceinline__ double loo_crps_pair(double w_u, double m, double h, double g) { return w_u * crps_abs_normal(m, h, g); }
__host__ __device__ __forceinline__ double loo_crps_self(double w_s, double g) { return w_s * (0.5 * g); }
// one sample's term of d_j: the side of crps_cdf_side, weighted
__host__ __device__ __forceinline__ double loo_crps_side(double w_s, bool above, double t) { return w_s * crps_cdf_side(above, t); }
// the value of a classifier's sample, the expression of k_dist_copy
__host__ __device__ __forceinline__ double loo_value_probit(double score) { return (erf(score * 0.70710678118654752440) + 1.0) / 2.0; }

// w = exp(lw) in place, once per (row, sample) of the tile (NaN stays NaN)
__global__ __launch_bounds__(WG) void k_loo_weights(double *__restrict__ lw, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t < n) lw[t] = exp(lw[t]);
}

// ---- the summary -----------------------------------------------------------------------------------------------------------------
struct RowLooSummaryArgs {
  const double *scores;  // [S][Tn] the tile's scores
  const double *w;       // [S][Tn] the normalised weights
  const double *aux;     // regression: 1 / alpha_s [S]; ordered probit: cut[S][n_cut]
  double *mean, *sd, *sd_y, *ess, *q;  // of the tile's first row (sd_y: regression only); q[n_q][ldq]
  int64_t Tn, ldq;
  int S, n_cut;
  int aux_lds;           // (ordered probit) the cutpoints are staged in LDS behind the rows
  int P, R;              // S padded to a power of two (0: no quantiles, no sort), rows per workgroup
  int st, stv, sti;      // doubles per row of w (S | 1) and of the values (max(S, P) | 1), ints per row of the sample indices (P | 1): odd
  int n_q;
  double p[DIST_MAX_Q];  // the probabilities, ascending
  int slot[DIST_MAX_Q];  // ... and where the caller listed each
};

// LDS, in doubles: val[R][stv], w[R][st], the sample indices idx[R][sti] (ints), the cutpoints where they are staged
static size_t loo_summary_lds_doubles(int R, int st, int stv, int sti, size_t n_aux) {
  return (size_t)R * ((size_t)st + (size_t)stv) + ((size_t)R * (size_t)sti + 1) / 2 + n_aux;
}

// Stage 3, one launch per row tile, in the LDS form of k_row_summary / k_row_psis. A workgroup brings R rows into LDS, every score
// turned into its value on the way (all threads). Lane r then walks row r in sample order three times: the mean, the second moment
// about it, and sum w^2 (regression: sum w / alpha as well, 1 / alpha_s at one address for all lanes). One bitonic network over
// P = S padded with +inf orders the (value, sample index) pairs of all R rows, ties by sample index; lane r then walks the order
// of row r once, adding w at the sample index, and resolves all n_q probabilities in that walk. The row strides are odd, that of
// the indices too: the row-per-lane phases are conflict-free but for the gather of w.
template <int TASK>
__global__ __launch_bounds__(WG) void k_row_loo_summary(RowLooSummaryArgs a) {
  extern __shared__ double loo_lds[];
  const int S = a.S, R = a.R, st = a.st, stv = a.stv, sti = a.sti, P = a.P, n_cut = a.n_cut;
  double *val = loo_lds, *w = val + (size_t)R * stv;
  int *idx = reinterpret_cast<int *>(w + (size_t)R * st);
  double *staged = w + (size_t)R * st + ((size_t)R * sti + 1) / 2;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(a.Tn - r0 < R ? a.Tn - r0 : R);
  const int tid = threadIdx.x;
  const bool use_staged = TASK == LOGDENS_ORDERED && a.aux_lds;
  if (use_staged) {
    for (int i = tid; i < S * n_cut; i += WG) staged[i] = a.aux[i];
    __syncthreads();
  }
  // (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto fill = [&](const double *cut) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      double x = 0.0, wv = 0.0;
      if (r < nr) {
        const double score = a.scores[(size_t)s * a.Tn + r0 + r];
        wv = a.w[(size_t)s * a.Tn + r0 + r];
        if constexpr (TASK == LOGDENS_REGRESSION)
          x = score;
        else if constexpr (TASK == LOGDENS_CLASSIFICATION)
          x = loo_value_probit(score);
        else
          x = oprobit_expected(score, cut + (size_t)s * n_cut, n_cut);
      }
      val[r * stv + s] = x;
      w[r * st + s] = wv;
      if (P) idx[r * sti + s] = s;
    }
  };
  if (use_staged)
    fill(staged);
  else
    fill(a.aux);
  for (int i = tid; i < (P - S) * R; i += WG) {  // (P = 0: no iteration)
    const int s = S + i / R, r = i % R;
    val[r * stv + s] = __builtin_inf();
    idx[r * sti + s] = s;
  }
  __syncthreads();
  bool nan_row = false;
  if (tid < nr) {
    const double *vr = val + tid * stv, *wr = w + tid * st;
    double mean = 0.0, m2 = 0.0, w2 = 0.0, nv = 0.0;
    for (int s = 0; s < S; s++) mean += wr[s] * vr[s];
    for (int s = 0; s < S; s++) {
      const double e = vr[s] - mean;
      m2 += wr[s] * (e * e);
    }
    for (int s = 0; s < S; s++) w2 += wr[s] * wr[s];
    nan_row = wr[0] != wr[0];
    a.mean[r0 + tid] = mean;
    a.sd[r0 + tid] = sqrt(m2);
    a.ess[r0 + tid] = 1.0 / w2;
    if constexpr (TASK == LOGDENS_REGRESSION) {
      for (int s = 0; s < S; s++) nv += wr[s] * a.aux[s];
      a.sd_y[r0 + tid] = sqrt(m2 + nv);
    }
  }
  if (!P) return;  // (one value for the grid)
  __syncthreads();  // (the moments read the values in sample order)
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < R * half; e += WG) {
        const int r = e / half, c2 = e - r * half;
        const int i = ((c2 & ~(j - 1)) << 1) | (c2 & (j - 1));
        double *vr = val + r * stv;
        int *ir = idx + r * sti;
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
  if (tid < nr) {
    const double *vr = val + tid * stv, *wr = w + tid * st;
    const int *ir = idx + tid * sti;
    double *out = a.q + r0 + tid;
    if (nan_row) {
      for (int q = 0; q < a.n_q; q++) out[(size_t)a.slot[q] * a.ldq] = __builtin_nan("");
    } else {
      loo_quantile_walk(
          S, [&](int i) { return vr[i]; },
          [&](int i) {
            const int si = ir[i];  // (a padding index can stand here only if a value was NaN: scores are finite)
            return si < S ? wr[si] : 0.0;
          },
          a.n_q, a.p, [&](int q, double x) { out[(size_t)a.slot[q] * a.ldq] = x; });
    }
  }
}

template <int TASK>
static void launch_row_loo_summary_form(hipStream_t s, const RowLooSummaryArgs &a, size_t lds) {
  static DeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {  // above the default limit of dynamic LDS (opted into once per device)
    void (*const kernel)(RowLooSummaryArgs) = k_row_loo_summary<TASK>;
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PSIS_LDS_MAX_BYTES));
    raised.mark();
  }
  hipLaunchKernelGGL((k_row_loo_summary<TASK>), dim3((unsigned)cdiv(a.Tn, a.R)), dim3(WG), lds, s, a);
}
// n_aux: the cutpoints of an ordered-probit call, in doubles. Sized by the arithmetic of launch_row_psis: R rows of
// (S | 1) + (max(S, P) | 1) doubles and (P | 1) ints within PSIS_LDS_BYTES, at most PSIS_MAX_ROWS and never less than one row
// (S = 4096 with quantiles: 10 243 doubles = 81 944 B, R = 1); the cutpoints behind them where the budget still holds them.
static void launch_row_loo_summary(hipStream_t s, int task, RowLooSummaryArgs &a, size_t n_aux) {
  int P = 0;
  if (a.n_q > 0) {
    P = 2;  // (S = 1: one pad, the network's one step leaves the value in front)
    while (P < a.S) P <<= 1;
  }
  a.P = P;
  a.st = a.S | 1;
  a.stv = std::max(a.S, P) | 1;
  a.sti = P ? P | 1 : 0;
  const size_t row = loo_summary_lds_doubles(1, a.st, a.stv, a.sti, 0);
  const size_t budget = PSIS_LDS_BYTES / sizeof(double);
  a.R = (int)std::min<int64_t>(std::max<int64_t>(1, std::min<int64_t>(PSIS_MAX_ROWS, (int64_t)(budget / row))), a.Tn);
  const size_t rows = loo_summary_lds_doubles(a.R, a.st, a.stv, a.sti, 0);
  a.aux_lds = task == LOGDENS_ORDERED && n_aux > 0 && rows + n_aux <= budget;
  const size_t lds = (rows + (a.aux_lds ? n_aux : 0)) * sizeof(double);
  logdens_with_task(task, [&](auto task_c) { launch_row_loo_summary_form<decltype(task_c)::value>(s, a, lds); });
}

// One row on the host, sequentially, through the scalar pieces and in the summation orders of k_row_loo_summary: values[S] (what
// the kernel forms from the score), lw[S] the normalised log weights, inv_alpha[S] or null, probs[n_q] in any order.
// out_q[n_q] in the order of probs; out_sd_y may be null.
static void loo_summary_row_host(int S, const double *values, const double *lw, const double *inv_alpha, int n_q, const double *probs,
                                 double *out_mean, double *out_sd, double *out_q, double *out_sd_y, double *out_ess) {
  std::vector<double> w((size_t)S);
  for (int s = 0; s < S; s++) w[(size_t)s] = exp(lw[s]);
  double mean = 0.0, m2 = 0.0, w2 = 0.0, nv = 0.0;
  for (int s = 0; s < S; s++) mean += w[(size_t)s] * values[s];
  for (int s = 0; s < S; s++) {
    const double e = values[s] - mean;
    m2 += w[(size_t)s] * (e * e);
  }
  for (int s = 0; s < S; s++) w2 += w[(size_t)s] * w[(size_t)s];
  *out_mean = mean;
  *out_sd = sqrt(m2);
  *out_ess = 1.0 / w2;
  if (out_sd_y) {
    for (int s = 0; s < S; s++) nv += w[(size_t)s] * inv_alpha[s];
    *out_sd_y = sqrt(m2 + nv);
  }
  if (n_q == 0) return;
  if (w[0] != w[0]) {
    std::fill(out_q, out_q + n_q, std::numeric_limits<double>::quiet_NaN());
    return;
  }
  std::vector<int> idx((size_t)S), slot((size_t)n_q);
  std::iota(idx.begin(), idx.end(), 0);
  std::sort(idx.begin(), idx.end(), [&](int i0, int i1) { return psis_after(values[i1], i1, values[i0], i0); });
  std::iota(slot.begin(), slot.end(), 0);
  std::stable_sort(slot.begin(), slot.end(), [&](int q0, int q1) { return probs[q0] < probs[q1]; });
  std::vector<double> p((size_t)n_q);
  for (int q = 0; q < n_q; q++) p[(size_t)q] = probs[slot[(size_t)q]];
  loo_quantile_walk(
      S, [&](int i) { return values[idx[(size_t)i]]; }, [&](int i) { return w[(size_t)idx[(size_t)i]]; }, n_q, p.data(),
      [&](int q, double x) { out_q[slot[(size_t)q]] = x; });
}

// ---- the CRPS ----------------------------------------------------------------------------------------------------------------------
struct RowLooCrpsArgs {
  const double *scores;  // [S][Tn] the tile's scores
  const double *w;       // [S][Tn] the normalised weights
  const double *y;       // of the tile's first row
  const double *aux;     // regression: crps_table_fill's constants; ordered probit: cut[S][n_cut]
  double *crps, *accuracy, *spread;  // of the tile's first row
  int64_t Tn;
  int S, n_cut;
  int aux_lds;           // (ordered probit) the cutpoints are staged in LDS (they fit LOGDENS_LDS_BYTES)
};

// Stage 3 for regression, the weighted form of k_row_crps_mix: a thread per row, the s axis blocked in registers. A lane holds the
// scores, the weights and the pair sums of B samples and streams (mu_u, w_u), u = 0 .. s - 1, once per block; the pair's (h, g) is
// read at a wave-uniform address. No LDS, no atomics. Pair sum s adds its terms in u order and its own term last, the pair sums
// are added in s order: a row's result depends on neither the tiling nor B.
template <int B>
__global__ __launch_bounds__(WG) void k_row_loo_crps_mix(RowLooCrpsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= a.Tn) return;
  const int S = a.S;
  const int64_t Tn = a.Tn;
  const double *__restrict__ col = a.scores + t;
  const double *__restrict__ wc = a.w + t;
  const double *__restrict__ own = a.aux;                  // (h, g) of v_s
  const double *__restrict__ tab = a.aux + 2 * (size_t)S;  // (h, g) of v_s + v_u
  const double yt = a.y[t];
  double acc = 0.0, total = 0.0;
  for (int s = 0; s < S; s++) acc += loo_crps_pair(wc[(size_t)s * Tn], yt - col[(size_t)s * Tn], own[2 * s], own[2 * s + 1]);
  for (int s0 = 0; s0 < S; s0 += B) {
    double mu[B], ws[B], p[B];
#pragma unroll
    for (int i = 0; i < B; i++) {
      mu[i] = s0 + i < S ? col[(size_t)(s0 + i) * Tn] : 0.0;
      ws[i] = s0 + i < S ? wc[(size_t)(s0 + i) * Tn] : 0.0;
      p[i] = 0.0;
    }
    const int u_end = (s0 + B < S ? s0 + B : S) - 1;  // the block's last sample pairs with u < u_end
    const int pair0 = s0 * (s0 + 1) / 2;              // of (s0, 0); row s + 1 of the table begins s + 1 entries behind row s
    for (int u = 0; u < u_end; u++) {
      const double mu_u = col[(size_t)u * Tn], w_u = wc[(size_t)u * Tn];
      int pair = pair0 + u;
#pragma unroll
      for (int i = 0; i < B; i++) {
        const int s = s0 + i;
        if (u < s && s < S) p[i] += loo_crps_pair(w_u, mu[i] - mu_u, tab[2 * pair], tab[2 * pair + 1]);
        pair += s + 1;
      }
    }
    int diag = pair0 + s0;  // of (s0, s0)
#pragma unroll
    for (int i = 0; i < B; i++) {
      const int s = s0 + i;
      if (s < S) {
        p[i] += loo_crps_self(ws[i], tab[2 * diag + 1]);
        total += ws[i] * p[i];
      }
      diag += s + 2;
    }
  }
  a.accuracy[t] = acc;
  a.spread[t] = total;
  a.crps[t] = acc - total;
}

// Stage 3 for classification and ordered probit, the weighted form of k_row_crps_cdf: a thread per row, the loop over the cuts
// outside the loop over the samples; the cutpoints from LDS while they fit, as there.
template <int TASK>
__global__ __launch_bounds__(WG) void k_row_loo_crps_cdf(RowLooCrpsArgs a) {
  extern __shared__ double loo_crps_lds[];
  const int S = a.S, n_cut = a.n_cut;
  const bool staged = TASK == LOGDENS_ORDERED && a.aux_lds;
  if (staged) {
    for (int i = threadIdx.x; i < S * n_cut; i += WG) loo_crps_lds[i] = a.aux[i];
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= a.Tn) return;
  const int64_t Tn = a.Tn;
  const double *__restrict__ col = a.scores + t;
  const double *__restrict__ wc = a.w + t;
  const double yt = a.y[t];
  // (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto run = [&](const double *cut) {
    double accuracy = 0.0, spread = 0.0, crps = 0.0;
    for (int j = 0; j < n_cut; j++) {
      const bool above = yt > (double)j;
      double d = 0.0;
      for (int s = 0; s < S; s++) {
        const double c = TASK == LOGDENS_ORDERED ? cut[(size_t)s * n_cut + j] : 0.0;
        d += loo_crps_side(wc[(size_t)s * Tn], above, c - col[(size_t)s * Tn]);
      }
      accuracy += d;
      spread += d * (1.0 - d);
      crps += d * d;
    }
    a.accuracy[t] = accuracy;
    a.spread[t] = spread;
    a.crps[t] = crps;
  };
  if (staged)
    run(loo_crps_lds);
  else
    run(a.aux);
}

static void launch_row_loo_crps(hipStream_t s, int task, const RowLooCrpsArgs &a) {
  const dim3 grid((unsigned)cdiv(a.Tn, WG));
  if (task == LOGDENS_REGRESSION) {
    hipLaunchKernelGGL(k_row_loo_crps_mix<LOO_CRPS_BLOCK>, grid, dim3(WG), 0, s, a);
  } else if (task == LOGDENS_CLASSIFICATION) {
    hipLaunchKernelGGL(k_row_loo_crps_cdf<LOGDENS_CLASSIFICATION>, grid, dim3(WG), 0, s, a);
  } else {
    const size_t lds = a.aux_lds ? (size_t)a.S * a.n_cut * sizeof(double) : 0;
    hipLaunchKernelGGL(k_row_loo_crps_cdf<LOGDENS_ORDERED>, grid, dim3(WG), lds, s, a);
  }
}

// One row on the host by the functions and in the orders of the two kernels: out = (crps, accuracy, spread). lw[S]: the normalised
// log weights; aux: crps_table_fill's constants (regression); cut[S][n_cut] (ordered probit).
static void loo_crps_row_host(int task, int S, double y, const double *scores, const double *lw, const double *aux, int n_cut, const double *cut,
                              double *out) {
  std::vector<double> w((size_t)S);
  for (int s = 0; s < S; s++) w[(size_t)s] = exp(lw[s]);
  if (task == LOGDENS_REGRESSION) {
    const double *tab = aux + 2 * (size_t)S;
    double acc = 0.0, total = 0.0;
    for (int s = 0; s < S; s++) acc += loo_crps_pair(w[(size_t)s], y - scores[s], aux[2 * (size_t)s], aux[2 * (size_t)s + 1]);
    for (int s = 0; s < S; s++) {
      const double *row = tab + (size_t)s * ((size_t)s + 1);
      double p = 0.0;
      for (int u = 0; u < s; u++) p += loo_crps_pair(w[(size_t)u], scores[s] - scores[u], row[2 * (size_t)u], row[2 * (size_t)u + 1]);
      p += loo_crps_self(w[(size_t)s], row[2 * (size_t)s + 1]);
      total += w[(size_t)s] * p;
    }
    out[1] = acc;
    out[2] = total;
    out[0] = acc - total;
    return;
  }
  double accuracy = 0.0, spread = 0.0, crps = 0.0;
  for (int j = 0; j < n_cut; j++) {
    const bool above = y > (double)j;
    double d = 0.0;
    for (int s = 0; s < S; s++)
      d += loo_crps_side(w[(size_t)s], above, (task == LOGDENS_ORDERED ? cut[(size_t)s * n_cut + j] : 0.0) - scores[s]);
    accuracy += d;
    spread += d * (1.0 - d);
    crps += d * d;
  }
  out[0] = crps;
  out[1] = accuracy;
  out[2] = spread;
}

// ---- the calls ---------------------------------------------------------------------------------------------------------------------
// what a call asks for on top of the leave-one-out weights: a summary (n_q, probs and its six outputs) or the CRPS (its four)
struct LooPredCall {
  bool crps;
  int32_t n_q;
  const double *probs;
  double *out_mean, *out_std, *out_q, *out_std_y, *out_ess;
  double *out_crps, *out_accuracy, *out_spread;
  double *out_k;
};

// the call in the words of a log density, for loo_check: three of its own outputs stand where lpd, elpd_loo and k^ do
static LogdensCall loo_pred_call(int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                                 int64_t tile_rows, int32_t chunk_samples, const LooPredCall &p) {
  return LogdensCall{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, p.crps ? p.out_crps : p.out_mean,
                     p.crps ? p.out_accuracy : p.out_std, p.out_k, nullptr, nullptr};
}

// Every argument check: loo_check, then the quantile checks of design_summary or the sample limit of crps_check. Nothing here
// touches the device.
static void loo_pred_check(const LogdensCall &c, const LooPredCall &p, int64_t N, int count, int32_t tail_len) {
  loo_check(c, N, count, tail_len);
  if (p.crps) {
    if (c.task == LOGDENS_REGRESSION && count > CRPS_MAX_S)
      throw Error(MFM_ERR_INVALID, "a regression CRPS is computed over at most " + std::to_string(CRPS_MAX_S) + " samples, got " + std::to_string(count));
    if (N > 0 && !p.out_spread) throw Error(MFM_ERR_INVALID, "a leave-one-out CRPS needs its four output arrays");
    return;
  }
  if (p.n_q < 0 || p.n_q > DIST_MAX_Q) throw Error(MFM_ERR_INVALID, "at most " + std::to_string(DIST_MAX_Q) + " quantiles per call");
  if (p.n_q > 0 && !p.probs) throw Error(MFM_ERR_INVALID, "quantiles asked for without their probabilities");
  for (int q = 0; q < p.n_q; q++)
    if (!(p.probs[q] >= 0.0 && p.probs[q] <= 1.0)) throw Error(MFM_ERR_INVALID, "quantile probability out of range ([0, 1]; with noise strictly inside)");
  if (p.out_std_y && c.task != LOGDENS_REGRESSION)
    throw Error(MFM_ERR_INVALID, "the predictive standard deviation of y is defined for regression (task 0) only");
  if (N > 0 && (!p.out_ess || (p.n_q > 0 && !p.out_q))) throw Error(MFM_ERR_INVALID, "a leave-one-out summary needs its output arrays");
}

static void design_loo_pred(mfm_design *d, const SampleView &v, const LogdensCall &c, int32_t tail_len, const LooPredCall &p) {
  const int count = v.count();
  check_sample_source(d, v);
  hipStream_t s = d->stream;
  const size_t N = (size_t)d->N;
  if (N == 0) return;
  // dist_out: lpd, elpd, k, pit of k_row_psis, then this call's own columns
  const size_t own = p.crps ? 3 : 4 + (size_t)p.n_q;
  const int64_t T = dist_tiles_reserve(d, v, c.tile_rows, N * (4 + own));
  if (d->loo_scores.n < (size_t)(T * count)) d->loo_scores.alloc((size_t)(T * count));
  const LogdensConstants k = logdens_upload(d, s, c, d->N, count);
  // this file's constants beside those of k_row_psis: the pair table (regression CRPS), 1 / alpha_s (regression summary)
  const double *own_aux = k.aux;
  if (c.task == LOGDENS_REGRESSION) {
    std::vector<double> aux;
    if (p.crps) {
      aux.resize(crps_table_size(count));
      crps_table_fill(c.precisions, count, aux.data());
    } else {
      aux.resize((size_t)count);
      for (int i = 0; i < count; i++) aux[(size_t)i] = 1.0 / c.precisions[i];
    }
    if (d->loo_aux.n < aux.size()) d->loo_aux.alloc(aux.size());
    MFM_HIP_CHECK(hipMemcpy(d->loo_aux.p, aux.data(), aux.size() * sizeof(double), hipMemcpyHostToDevice));
    own_aux = d->loo_aux.p;
  }
  RowPsisArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scratch = d->dist_scratch.p;
  a.aux = k.aux;
  a.S = count;
  a.n_cut = c.task == LOGDENS_ORDERED ? c.n_cut : 0;
  a.M = tail_len;
  a.log_S = std::log((double)count);
  double *const out = d->dist_out.p + 4 * N;
  RowLooSummaryArgs sa;
  RowLooCrpsArgs ca;
  std::memset(&sa, 0, sizeof(sa));
  std::memset(&ca, 0, sizeof(ca));
  if (p.crps) {
    ca.scores = d->loo_scores.p;
    ca.w = d->dist_scratch.p;
    ca.aux = own_aux;
    ca.S = count;
    ca.n_cut = c.task == LOGDENS_ORDERED ? c.n_cut : 1;  // (a classifier: the one cutpoint 0)
    ca.aux_lds = c.task == LOGDENS_ORDERED && k.n_aux * sizeof(double) <= (size_t)LOGDENS_LDS_BYTES;
  } else {
    sa.scores = d->loo_scores.p;
    sa.w = d->dist_scratch.p;
    sa.aux = own_aux;
    sa.ldq = (int64_t)N;
    sa.S = count;
    sa.n_cut = a.n_cut;
    sa.n_q = p.n_q;
    std::vector<int> slot((size_t)p.n_q);  // the probabilities ascending, once; the results go to the caller's places
    std::iota(slot.begin(), slot.end(), 0);
    std::stable_sort(slot.begin(), slot.end(), [&](int q0, int q1) { return p.probs[q0] < p.probs[q1]; });
    for (int q = 0; q < p.n_q; q++) {
      sa.p[q] = p.probs[slot[(size_t)q]];
      sa.slot[q] = slot[(size_t)q];
    }
  }
  const bool pit = c.task == LOGDENS_REGRESSION;
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    const size_t n = (size_t)Tn * (size_t)count;
    MFM_HIP_CHECK(hipMemcpyAsync(d->loo_scores.p, d->dist_scratch.p, n * sizeof(double), hipMemcpyDeviceToDevice, s));
    a.Tn = Tn;
    a.y = d->dist_y.p + r0;
    a.lpd = d->dist_out.p + r0;
    a.elpd = d->dist_out.p + N + r0;
    a.khat = d->dist_out.p + 2 * N + r0;
    a.pit = pit ? d->dist_out.p + 3 * N + r0 : nullptr;
    launch_row_psis(s, c.task, a, k.n_aux, true);
    hipLaunchKernelGGL(k_loo_weights, dim3((unsigned)cdiv((int64_t)n, WG)), dim3(WG), 0, s, d->dist_scratch.p, (int64_t)n);
    if (p.crps) {
      ca.Tn = Tn;
      ca.y = d->dist_y.p + r0;
      ca.crps = out + r0;
      ca.accuracy = out + N + r0;
      ca.spread = out + 2 * N + r0;
      launch_row_loo_crps(s, c.task, ca);
    } else {
      sa.Tn = Tn;
      sa.mean = out + r0;
      sa.sd = out + N + r0;
      sa.sd_y = out + 2 * N + r0;
      sa.ess = out + 3 * N + r0;
      sa.q = out + 4 * N + r0;
      launch_row_loo_summary(s, c.task, sa, k.n_aux);
    }
  };
  if (p.crps)
    dist_tiles_run(d, v, T, 0, c.chunk_samples, nullptr,
                   {{p.out_k, 2 * N, N}, {p.out_crps, 4 * N, N}, {p.out_accuracy, 5 * N, N}, {p.out_spread, 6 * N, N}}, stage2);
  else
    dist_tiles_run(d, v, T, 0, c.chunk_samples, nullptr,
                   {{p.out_k, 2 * N, N}, {p.out_mean, 4 * N, N}, {p.out_std, 5 * N, N}, {p.out_std_y, 6 * N, pit && p.out_std_y ? N : 0},
                    {p.out_ess, 7 * N, N}, {p.out_q, 8 * N, N * (size_t)p.n_q}},
                   stage2);
}

static LooPredCall loo_summary_call(int32_t n_q, const double *probs, double *out_mean, double *out_std, double *out_q, double *out_std_y,
                                    double *out_ess, double *out_k) {
  return LooPredCall{false, n_q, probs, out_mean, out_std, out_q, out_std_y, out_ess, nullptr, nullptr, nullptr, out_k};
}
static LooPredCall loo_crps_call(double *out_crps, double *out_accuracy, double *out_spread, double *out_k) {
  return LooPredCall{true, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out_crps, out_accuracy, out_spread, out_k};
}

}  // namespace mfm

extern "C" {

int mfm_design_loo_summary_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                                 const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                                 int32_t tail_len, int32_t n_q, const double *probs, double *out_mean, double *out_std, double *out_q,
                                 double *out_std_y, double *out_ess, double *out_k) {
  MFM_TRY(d)
  const mfm::LooPredCall p = mfm::loo_summary_call(n_q, probs, out_mean, out_std, out_q, out_std_y, out_ess, out_k);
  const LogdensCall c = loo_pred_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, p);
  loo_pred_check(c, p, d->N, std::max(count, 0), tail_len);
  design_loo_pred(d, samples_of_store(st, first, count), c, tail_len, p);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_loo_summary(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t task,
                           const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                           int32_t chunk_samples, int32_t tail_len, int32_t n_q, const double *probs, double *out_mean, double *out_std,
                           double *out_q, double *out_std_y, double *out_ess, double *out_k) {
  MFM_TRY(d)
  const mfm::LooPredCall p = mfm::loo_summary_call(n_q, probs, out_mean, out_std, out_q, out_std_y, out_ess, out_k);
  const LogdensCall c = loo_pred_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, p);
  loo_pred_check(c, p, d->N, std::max(n_samples, 0), tail_len);
  store_check_fraction(d->D, rank, n_samples);
  design_loo_pred(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), c, tail_len, p);
  MFM_CATCH(d)
}

int mfm_design_loo_crps_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                              const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                              int32_t tail_len, double *out_crps, double *out_accuracy, double *out_spread, double *out_k) {
  MFM_TRY(d)
  const mfm::LooPredCall p = mfm::loo_crps_call(out_crps, out_accuracy, out_spread, out_k);
  const LogdensCall c = loo_pred_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, p);
  loo_pred_check(c, p, d->N, std::max(count, 0), tail_len);
  design_loo_pred(d, samples_of_store(st, first, count), c, tail_len, p);
  MFM_CATCH(d)
}

int mfm_design_loo_crps(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t task,
                        const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                        int32_t chunk_samples, int32_t tail_len, double *out_crps, double *out_accuracy, double *out_spread, double *out_k) {
  MFM_TRY(d)
  const mfm::LooPredCall p = mfm::loo_crps_call(out_crps, out_accuracy, out_spread, out_k);
  const LogdensCall c = loo_pred_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, p);
  loo_pred_check(c, p, d->N, std::max(n_samples, 0), tail_len);
  store_check_fraction(d->D, rank, n_samples);
  design_loo_pred(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), c, tail_len, p);
  MFM_CATCH(d)
}

// one row of k_row_loo_summary on the host, by the scalar pieces the kernel runs (no device): values[S] and log_weights[S],
// 1 <= S <= 4096; inv_alpha[S] with out_std_y, else both NULL; out_q[n_q] in the order of probs
int mfm_loo_summary_row(int32_t S, const double *values, const double *log_weights, const double *inv_alpha, int32_t n_q, const double *probs,
                        double *out_mean, double *out_std, double *out_q, double *out_std_y, double *out_ess) {
  try {
    if (S < 1 || S > mfm::DIST_MAX_S || !values || !log_weights || !out_mean || !out_std || !out_ess)
      throw mfm::Error(MFM_ERR_INVALID, "a row of 1 to " + std::to_string(mfm::DIST_MAX_S) + " values and log weights and the outputs are needed");
    if (n_q < 0 || n_q > mfm::DIST_MAX_Q) throw mfm::Error(MFM_ERR_INVALID, "at most " + std::to_string(mfm::DIST_MAX_Q) + " quantiles per call");
    if (n_q > 0 && (!probs || !out_q)) throw mfm::Error(MFM_ERR_INVALID, "quantiles asked for without their probabilities");
    for (int q = 0; q < n_q; q++)
      if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
        throw mfm::Error(MFM_ERR_INVALID, "quantile probability out of range ([0, 1]; with noise strictly inside)");
    if ((inv_alpha != nullptr) != (out_std_y != nullptr))
      throw mfm::Error(MFM_ERR_INVALID, "inv_alpha and out_std_y are given together (regression) or not at all");
    for (int s = 0; s < S; s++)
      if (!std::isfinite(values[s])) throw mfm::Error(MFM_ERR_INVALID, "values must be finite");
    mfm::loo_summary_row_host(S, values, log_weights, inv_alpha, n_q, probs, out_mean, out_std, out_q, out_std_y, out_ess);
  } catch (const mfm::Error &e) {
    g_global_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_global_error = "host out of memory";
    return MFM_ERR_RUNTIME;
  }
  return MFM_OK;
}

// one row of the two CRPS kernels on the host, by the functions they run and in their summation orders: out = (crps, accuracy, spread)
int mfm_loo_crps_row(int32_t task, int32_t S, double y, const double *scores, const double *log_weights, const double *precisions, int32_t n_cut,
                     const double *cutpoints, double *out) {
  try {
    if (S < 1 || !scores || !log_weights || !out)
      throw mfm::Error(MFM_ERR_INVALID, "a row of at least one score and log weight and the output of three values are needed");
    mfm::crps_check(mfm::crps_call(task, &y, precisions, n_cut, cutpoints, 0, 0, out, out + 1, out + 2), 1, S);
    if (S > mfm::DIST_MAX_S)
      throw mfm::Error(MFM_ERR_INVALID, "leave-one-out weights are computed over at most " + std::to_string(mfm::DIST_MAX_S) + " samples, got " + std::to_string(S));
    for (int s = 0; s < S; s++)
      if (!std::isfinite(scores[s])) throw mfm::Error(MFM_ERR_INVALID, "scores must be finite");
    std::vector<double> aux;
    if (task == mfm::LOGDENS_REGRESSION) {
      aux.resize(mfm::crps_table_size(S));
      mfm::crps_table_fill(precisions, S, aux.data());
    }
    mfm::loo_crps_row_host(task, S, y, scores, log_weights, aux.data(), task == mfm::LOGDENS_ORDERED ? n_cut : 1, cutpoints, out);
  } catch (const mfm::Error &e) {
    g_global_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_global_error = "host out of memory";
    return MFM_ERR_RUNTIME;
  }
  return MFM_OK;
}

}  // extern "C"
