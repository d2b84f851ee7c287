// mfm_logdens.hpp -- pointwise log predictive density over the kept samples (not in the reference): per test row the
// log of the posterior-mean density of the observed target, lpd = logsumexp_s l_s - log S with l_s = log p(y | theta_s), the mean and
// the sample variance (ddof = 1, WAIC's penalty) of the l_s, for regression the probability integral transform
// mean_s Phi((y - score_s) sqrt(alpha_s)), and on request the l_s themselves. Included by mfm_hip.hip after mfm_dist.hpp.
//
// Rows are processed by the tiled pass of mfm_dist.hpp (dist_tiles_run): its stage 1 leaves the scores of a tile sample-major in
// the scratch [S][T], the stage 2 given to it here, k_row_logdens, walks every row's samples in sample order. Everything is fp64, there
// are no atomics: a rerun, another row tile or another sample chunk give the same bits.
#pragma once
#include "mfm_erfcx.hpp"

namespace mfm {

constexpr int LOGDENS_REGRESSION = 0, LOGDENS_CLASSIFICATION = 1, LOGDENS_ORDERED = 2;  // (the values of TaskType)

// log(Phi(hi) - Phi(lo)) of the standard normal, lo = -inf / hi = +inf where has_lo / has_hi is false: the arithmetic of
// k_oprobit_eval (mfm_tasks.hpp), without its gradient and Hessian terms. With x = hi, yv = lo, E(t) = erfcx(|t| / sqrt 2),
// g(t) = exp(-t^2 / 2):
//   A (yv > 0):        2 (Phi(x) - Phi(yv)) = g(yv) [E(yv) - ef E(x)],  ef = exp((yv^2 - x^2) / 2)
//   B (x < 0):                             = g(x)  [E(x) - ef E(yv)],  ef = exp((x^2 - yv^2) / 2)
//   C (yv <= 0 <= x):                      = 2 - g(x) E(x) - g(yv) E(yv)
// one evaluation for all lanes of a wavefront, whatever their labels: 2 erfcx, 2 exp, 1 log. A and B never form Phi, so the
// result stays finite and relatively accurate where Phi underflows (|t| ~ 38). In C the log is taken as log1p(-(gE(x) + gE(yv)) / 2):
// the log of the rounded 1 - d would lose the relative accuracy of a log density near 0 (d ~ 1e-16 at t = 8). A narrow
// interval around 0 (both ends within 0.5) cancels in C; there erf(x / sqrt 2) - erf(yv / sqrt 2) keeps full relative accuracy.
__host__ __device__ __forceinline__ double logdens_interval(bool has_lo, double yv, bool has_hi, double x) {
  const double SQRT2 = 1.4142135623730951;
  x = has_hi ? x : 0.0;
  yv = has_lo ? yv : 0.0;
  const bool cA = has_lo && yv > 0, cB = !cA && has_hi && x < 0, cC = !cA && !cB;
  double Ex = d_erfcx_pos(has_hi ? fabs(x) / SQRT2 : 1.0), Ey = d_erfcx_pos(has_lo ? fabs(yv) / SQRT2 : 1.0);
  Ex = has_hi ? Ex : 0.0;
  Ey = has_lo ? Ey : 0.0;
  const double hx = x * x / 2, hy = yv * yv / 2;
  const double a1 = cA ? hy - hx : (cB ? 0.0 : -hx), a2 = cA ? 0.0 : (cB ? hx - hy : -hy);
  double f_hi = exp(has_hi ? a1 : 0.0), f_lo = exp(has_lo ? a2 : 0.0);
  f_hi = has_hi ? f_hi : 0.0;
  f_lo = has_lo ? f_lo : 0.0;
  const double pa = f_hi * Ex, pb = f_lo * Ey;
  double den = cC ? 2.0 - (pa + pb) : (cA ? pb - pa : pa - pb);
  const bool narrow = cC && has_hi && has_lo && fmax(fabs(x), fabs(yv)) < 0.5;
  if (narrow) den = erf(x / SQRT2) - erf(yv / SQRT2);
  // C outside the narrow form: log1p(u), u = -(gE(x) + gE(yv)) / 2, from the one log as log(w) u / (w - 1) with w the rounded 1 + u
  // (the quotient undoes the rounding of w; w = 1: log1p(u) = u to its last bit)
  const bool wide = cC && !narrow;
  const double u = -((pa + pb) / 2), w = 1.0 + u;
  const double lg = log(wide ? w : den / 2);
  const double l1p = w == 1.0 ? u : lg * (u / (w - 1.0));
  const double L = cA ? -hy : (cB ? -hx : 0.0);
  return L + (wide ? l1p : lg);
}

// l = log p(y | score, the sample's constants):
//   regression       log_norm - z^2 / 2, z = (y - score) sqrt_alpha, log_norm = log(alpha) / 2 - log(2 pi) / 2 (once per sample, host)
//   classification   log Phi(score) for y = 1, log Phi(-score) for y = 0: the one-sided limits of the interval
//   ordered probit   log(Phi(cut[y] - score) - Phi(cut[y - 1] - score)), cut[-1] = -inf, cut[n_cut] = +inf; cut: the sample's row
template <int TASK>
__host__ __device__ __forceinline__ double logdens_value(double y, double score, double log_norm, double sqrt_alpha, const double *cut,
                                                         int n_cut) {
  if constexpr (TASK == LOGDENS_REGRESSION) {
    const double z = (y - score) * sqrt_alpha;
    return log_norm - z * z / 2;
  } else if constexpr (TASK == LOGDENS_CLASSIFICATION) {
    return logdens_interval(false, 0.0, true, y > 0.5 ? score : -score);
  } else {
    const int label = (int)y;
    const bool has_lo = label > 0, has_hi = label < n_cut;
    return logdens_interval(has_lo, has_lo ? cut[label - 1] - score : 0.0, has_hi, has_hi ? cut[label] - score : 0.0);
  }
}

// One step of the streaming log-sum-exp in sample order, for sample s with value l: the running maximum m and acc = sum exp(l - m),
// rescaled when m moves, one exp per sample; lpd = m + log(acc) - log S. The one text of k_row_logdens and of k_row_psis
// (mfm_psis.hpp), which must give lpd the same bits. A macro and not a function: as an inlined function the same statements left
// k_row_logdens with other registers and another instruction order than the parent commit's, as a macro its listing is the
// parent's instruction for instruction.
#define MFM_LOGDENS_LSE_STEP(s, l, m, acc)                                                                                  \
  if (s == 0) {                                                                                                             \
    m = l;                                                                                                                  \
    acc = 1.0;                                                                                                              \
  } else {                                                                                                                  \
    const double e = l == m ? 1.0 : exp(-fabs(l - m)); /* (l = m = -inf: a density of 0 under every sample so far) */      \
    acc = l > m ? acc * e + 1.0 : acc + e;                                                                                  \
    m = fmax(m, l);                                                                                                         \
  }

struct RowLogdensArgs {
  double *scratch;    // [S][Tn] the tile's scores; KEEP: l in their place on exit
  const double *y;    // of the tile's first row
  const double *aux;  // the per-sample constants -- regression: log_norm[S] then sqrt(alpha)[S]; ordered probit: cut[S][n_cut]
  double *lpd, *mean, *var, *pit;  // of the tile's first row (pit: regression only)
  int64_t Tn;
  int S, n_cut;
  int aux_lds;        // the constants are staged in LDS (they fit LOGDENS_LDS_BYTES)
  double inv_S, inv_Sm1, log_S;  // 1 / S, 1 / (S - 1) (0 for S = 1), log S
};
constexpr int LOGDENS_LDS_BYTES = 48 * 1024;

// Stage 2, one launch per row tile: a thread per row (consecutive lanes read consecutive scratch[s][t] and y[t]). The loop over
// the samples folds l_s into a streaming log-sum-exp (the running maximum m and sum_s exp(l_s - m), rescaled when m moves: one
// exp per sample), into the plain sum (the mean, added as the predictors add) and into Welford's update of the squared
// deviations (exactly 0 for equal values; a row's result depends on its own samples alone, so not on the tiling). The per-sample
// constants are read from LDS, staged once per workgroup, or -- where they do not fit -- from global memory at one address per
// sample for the whole workgroup (ordered probit: one of n_cut + 1 addresses, by the lane's label).
template <int TASK, bool KEEP>
__global__ __launch_bounds__(WG) void k_row_logdens(RowLogdensArgs a) {
  extern __shared__ double logdens_lds[];
  const int S = a.S, n_cut = a.n_cut;
  const bool staged = TASK != LOGDENS_CLASSIFICATION && a.aux_lds;
  if (staged) {
    const int n_aux = TASK == LOGDENS_REGRESSION ? 2 * S : S * n_cut;
    for (int i = threadIdx.x; i < n_aux; i += WG) logdens_lds[i] = a.aux[i];
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= a.Tn) return;
  const int64_t Tn = a.Tn;
  double *__restrict__ col = a.scratch + t;
  const double yt = a.y[t];
  // (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto run = [&](const double *aux) {
    double m = 0.0, acc = 0.0, sum = 0.0, wmean = 0.0, m2 = 0.0, pit = 0.0;
    for (int s = 0; s < S; s++) {
      const double score = col[(size_t)s * Tn];
      double l;
      if constexpr (TASK == LOGDENS_REGRESSION) {
        const double sqa = aux[S + s];
        l = logdens_value<TASK>(yt, score, aux[s], sqa, nullptr, 0);
        pit += 0.5 * erfc(-((yt - score) * sqa) * 0.70710678118654752440);
      } else if constexpr (TASK == LOGDENS_CLASSIFICATION) {
        l = logdens_value<TASK>(yt, score, 0.0, 0.0, nullptr, 0);
      } else {
        l = logdens_value<TASK>(yt, score, 0.0, 0.0, aux + (size_t)s * n_cut, n_cut);
      }
      if (KEEP) col[(size_t)s * Tn] = l;
      MFM_LOGDENS_LSE_STEP(s, l, m, acc)
      sum += l;
      const double delta = l - wmean;
      wmean += delta / (double)(s + 1);
      m2 += delta * (l - wmean);
    }
    a.lpd[t] = m + log(acc) - a.log_S;
    a.mean[t] = sum * a.inv_S;
    a.var[t] = m2 * a.inv_Sm1;
    if constexpr (TASK == LOGDENS_REGRESSION) a.pit[t] = pit * a.inv_S;
  };
  if (staged)
    run(logdens_lds);
  else
    run(a.aux);
}

// The runtime task (checked: one of the three) as a compile-time constant: f(std::integral_constant<int, TASK>{}). The one dispatch
// of launch_row_logdens, of launch_row_psis (mfm_psis.hpp) and of mfm_logdens_value.
template <class F>
static auto logdens_with_task(int task, const F &f) {
  if (task == LOGDENS_REGRESSION) return f(std::integral_constant<int, LOGDENS_REGRESSION>{});
  if (task == LOGDENS_CLASSIFICATION) return f(std::integral_constant<int, LOGDENS_CLASSIFICATION>{});
  return f(std::integral_constant<int, LOGDENS_ORDERED>{});
}

static void launch_row_logdens(hipStream_t s, int task, const RowLogdensArgs &a, bool keep) {
  const size_t n_aux = task == LOGDENS_REGRESSION ? 2 * (size_t)a.S : task == LOGDENS_ORDERED ? (size_t)a.S * a.n_cut : 0;
  const size_t lds = a.aux_lds ? n_aux * sizeof(double) : 0;
  const dim3 grid((unsigned)cdiv(a.Tn, WG));
  logdens_with_task(task, [&](auto task_c) {
    constexpr int TASK = decltype(task_c)::value;
    if (keep)
      hipLaunchKernelGGL((k_row_logdens<TASK, true>), grid, dim3(WG), lds, s, a);
    else
      hipLaunchKernelGGL((k_row_logdens<TASK, false>), grid, dim3(WG), lds, s, a);
  });
}

// what a call computes besides the samples: the task, the targets y[N] and that task's per-sample constants, all on the host
struct LogdensCall {
  int32_t task;
  const double *y, *precisions;  // precisions[S]: regression
  int32_t n_cut;
  const double *cutpoints;       // [S][n_cut]: ordered probit
  int64_t tile_rows;
  int32_t chunk_samples;
  double *out_lpd, *out_mean, *out_var, *out_pit, *out_ll;  // [N] each, out_pit (regression) and out_ll[S][N] optional
};

// Every argument check of a call over `count` samples and N rows; nothing here touches the device.
static void logdens_check(const LogdensCall &c, int64_t N, int count) {
  if (c.task < 0 || c.task > 2) throw Error(MFM_ERR_INVALID, "bad task (0: regression, 1: probit classification, 2: ordered probit)");
  check_tiling(c.tile_rows, c.chunk_samples);
  if (c.task == LOGDENS_REGRESSION) {
    if (!c.precisions) throw Error(MFM_ERR_INVALID, "a regression log density needs the noise precision of every sample");
    check_precisions(c.precisions, count);
  } else if (c.precisions) {
    throw Error(MFM_ERR_INVALID, "noise precisions apply to regression (task 0) only");
  }
  if (c.task == LOGDENS_ORDERED) {
    if (c.n_cut < 1) throw Error(MFM_ERR_INVALID, "an ordered-probit log density needs at least one cutpoint per sample");
    if (!c.cutpoints) throw Error(MFM_ERR_INVALID, "an ordered-probit log density needs the samples' cutpoints");
    check_cutpoints(c.cutpoints, count, c.n_cut);
  } else if (c.cutpoints || c.n_cut != 0) {
    throw Error(MFM_ERR_INVALID, "cutpoints apply to ordered probit (task 2) only");
  }
  if (c.out_pit && c.task != LOGDENS_REGRESSION) throw Error(MFM_ERR_INVALID, "the probability integral transform is defined for regression (task 0) only");
  if (N == 0) return;
  if (!c.y) throw Error(MFM_ERR_INVALID, "a log density needs the observed targets");
  if (!c.out_lpd || !c.out_mean || !c.out_var) throw Error(MFM_ERR_INVALID, "a log density needs its three output arrays");
  for (int64_t t = 0; t < N; t++) {
    const double y = c.y[t];
    if (!std::isfinite(y)) throw Error(MFM_ERR_INVALID, "y must be finite");
    if (c.task == LOGDENS_CLASSIFICATION && y != 0.0 && y != 1.0) throw Error(MFM_ERR_INVALID, "classification labels must be 0 or 1");
    // (the range first: inside it the cast is exact, and the loop calls nothing -- with a floor per row its time followed its address)
    if (c.task == LOGDENS_ORDERED && (y < 0.0 || y > (double)c.n_cut || y != (double)(int)y))
      throw Error(MFM_ERR_INVALID, "ordered-probit labels must be integers in [0, n_cut]");
  }
}

// The targets of the N rows into d->dist_y and the task's per-sample constants onto the device (design_logdens, and design_loo of
// mfm_psis.hpp): where they are, and how many doubles.
struct LogdensConstants {
  const double *aux;
  size_t n_aux;
};
static LogdensConstants logdens_upload(mfm_design *d, hipStream_t s, const LogdensCall &c, int64_t N, int count) {
  if (d->dist_y.n < (size_t)N) d->dist_y.alloc((size_t)N);
  MFM_HIP_CHECK(hipMemcpyAsync(d->dist_y.p, c.y, (size_t)N * sizeof(double), hipMemcpyHostToDevice, s));
  if (c.task == LOGDENS_REGRESSION) {
    const size_t n_aux = 2 * (size_t)count;
    std::vector<double> aux(n_aux);
    for (int k = 0; k < count; k++) {
      aux[(size_t)k] = 0.5 * std::log(c.precisions[k]) - 0.91893853320467274178;  // log(2 pi) / 2
      aux[(size_t)count + k] = std::sqrt(c.precisions[k]);
    }
    if (d->dist_aux.n < n_aux) d->dist_aux.alloc(n_aux);
    MFM_HIP_CHECK(hipMemcpy(d->dist_aux.p, aux.data(), n_aux * sizeof(double), hipMemcpyHostToDevice));
    return {d->dist_aux.p, n_aux};
  }
  if (c.task == LOGDENS_ORDERED) {
    const size_t n_aux = (size_t)count * c.n_cut;
    if (d->cut.n < n_aux) d->cut.alloc(n_aux);
    MFM_HIP_CHECK(hipMemcpyAsync(d->cut.p, c.cutpoints, n_aux * sizeof(double), hipMemcpyHostToDevice, s));
    return {d->cut.p, n_aux};
  }
  return {nullptr, 0};
}

static void design_logdens(mfm_design *d, const SampleView &v, const LogdensCall &c) {
  const int count = v.count();
  check_sample_source(d, v);
  hipStream_t s = d->stream;
  const size_t N = (size_t)d->N;
  if (N == 0) return;
  const bool pit = c.task == LOGDENS_REGRESSION;
  const int64_t T = dist_tiles_reserve(d, v, c.tile_rows, N * (pit ? 4 : 3));  // lpd, mean, var, pit
  const LogdensConstants k = logdens_upload(d, s, c, d->N, count);
  RowLogdensArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scratch = d->dist_scratch.p;
  a.S = count;
  a.inv_S = 1.0 / count;
  a.inv_Sm1 = count > 1 ? 1.0 / (count - 1) : 0.0;
  a.log_S = std::log((double)count);
  a.aux = k.aux;
  a.n_cut = c.task == LOGDENS_ORDERED ? c.n_cut : 0;
  a.aux_lds = k.n_aux > 0 && k.n_aux * sizeof(double) <= (size_t)LOGDENS_LDS_BYTES;
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    a.Tn = Tn;
    a.y = d->dist_y.p + r0;
    a.lpd = d->dist_out.p + r0;
    a.mean = d->dist_out.p + N + r0;
    a.var = d->dist_out.p + 2 * N + r0;
    a.pit = pit ? d->dist_out.p + 3 * N + r0 : nullptr;
    launch_row_logdens(s, c.task, a, c.out_ll != nullptr);
  };
  // out_ll: the tile's l, which KEEP leaves in the scratch
  dist_tiles_run(d, v, T, 0, c.chunk_samples, c.out_ll,
                 {{c.out_lpd, 0, N}, {c.out_mean, N, N}, {c.out_var, 2 * N, N}, {c.out_pit, 3 * N, pit && c.out_pit ? N : 0}}, stage2);
}

}  // namespace mfm

extern "C" {

int mfm_design_logdens_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                             const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                             double *out_lpd, double *out_mean, double *out_var, double *out_pit, double *out_ll) {
  MFM_TRY(d)
  const LogdensCall c{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_lpd, out_mean, out_var, out_pit, out_ll};
  logdens_check(c, d->N, std::max(count, 0));
  design_logdens(d, samples_of_store(st, first, count), c);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_logdens(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t task,
                       const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                       int32_t chunk_samples, double *out_lpd, double *out_mean, double *out_var, double *out_pit, double *out_ll) {
  MFM_TRY(d)
  const LogdensCall c{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_lpd, out_mean, out_var, out_pit, out_ll};
  logdens_check(c, d->N, std::max(n_samples, 0));
  store_check_fraction(d->D, rank, n_samples);
  design_logdens(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), c);
  MFM_CATCH(d)
}

// logdens_value on the host, by the code the kernel runs: l of one (y, score) under one sample's constants; cutpoints_row[n_cut]
int mfm_logdens_value(int32_t task, double y, double score, double log_norm, double sqrt_alpha, int32_t n_cut, const double *cutpoints_row,
                      double *out) {
  const bool label_ok = n_cut >= 1 && cutpoints_row && y >= 0.0 && y <= (double)n_cut;
  if (task < 0 || task > 2 || (task == mfm::LOGDENS_ORDERED && !label_ok)) {
    g_global_error = "bad task, or an ordered-probit label outside its cutpoints";
    return MFM_ERR_INVALID;
  }
  // every task is handed all the constants: the if constexpr branches of logdens_value read their own task's alone
  *out = mfm::logdens_with_task(task, [&](auto task_c) {
    return mfm::logdens_value<decltype(task_c)::value>(y, score, log_norm, sqrt_alpha, cutpoints_row, n_cut);
  });
  return MFM_OK;
}

}  // extern "C"
