// mfm_dist.hpp -- posterior predictive summaries (not in the reference): per test row the mean, the population
// standard deviation and empirical quantiles of the S kept samples' values (score, or Phi(score)), and with per-sample noise
// precisions the moments and quantiles of the mixture mean_s N(score_s, 1 / alpha_s). Ordered probit: the values are the class
// probabilities p_c(score_s; cutpoints_s), one summary per (row, class), or the expected class index sum_c c p_c; both are taken
// from the stored scores where stage 2 reads them (the load transform of k_row_summary). Included by mfm_hip.hip after
// mfm_predict.hpp.
//
// Rows are processed in tiles of T rows (dist_tiles_run, the one tiled pass of this file, mfm_logdens.hpp and mfm_psis.hpp).
// Stage 1 writes the values of a tile, all samples, into a sample-major scratch [S][T] (k_score_store MODE 3 / 4, or the
// per-sample pass and k_dist_copy for designs with relation blocks); stage 2, here k_row_summary, reduces every row of the tile.
// Everything is fp64, there are no atomics, every sum runs in sample order.
#pragma once

namespace mfm {

constexpr int DIST_MAX_Q = 32;             // quantiles per call
constexpr int DIST_MAX_S = 4096;           // samples per call when quantiles are asked for (a row's values are sorted in LDS)
constexpr size_t DIST_SCRATCH_BYTES = (size_t)256 << 20;
constexpr int DIST_LDS_BYTES = 48 * 1024;  // per workgroup, where more than one row fits
constexpr int DIST_LDS_MAX_BYTES = (2 * DIST_MAX_S + 1) * 8;  // one row of DIST_MAX_S samples and their sqrt(alpha)
constexpr int DIST_MAX_ROWS = 32;          // rows per workgroup of the LDS form

// scratch[t] = score[t] | Phi(score[t]) (the expression of k_accumulate_pred): one sample's slot of a row tile
__global__ __launch_bounds__(WG) void k_dist_copy(const double *__restrict__ score, double *__restrict__ scratch, int64_t n, int mode) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= n) return;
  double v = score[t];
  if (mode == 1) v = (erf(v * 0.70710678118654752440) + 1.0) / 2.0;
  scratch[t] = v;
}

struct RowSummaryArgs {
  const double *scratch;  // [S][Tn]
  const double *sqa;      // [S] sqrt(alpha_s) (noise)
  double *mean, *sd, *q;  // of the tile's first row; q[n_q][ldq]
  int64_t Tn, ldq;
  int S, P, stride, R;    // P: S padded to a power of two (sorted form), stride: doubles per row in LDS, R: rows per workgroup
  int n_q, noise;
  double inv_S, noise_var;  // 1 / S, mean_s 1 / alpha_s
  int lo[DIST_MAX_Q];       // empirical: the lower order statistic of quantile q ...
  double g[DIST_MAX_Q];     // ... and the weight of the upper one; noise: Phi^-1(p_q)
  double p[DIST_MAX_Q];
};

// The load transforms of stage 2: what a stored score becomes on its way out of the scratch.
constexpr int XF_NONE = 0;      // the stored value itself
constexpr int XF_CLASS = 1;     // p_c(score; the sample's cutpoints), class c = c0 + blockIdx.y; outputs strided by C
constexpr int XF_EXPECTED = 2;  // sum_c c p_c
struct RowTransformArgs {
  const double *cut;  // [S][n_cut], on the device
  int n_cut, C;       // C: values per row in the outputs (XF_CLASS: n_cut + 1, XF_EXPECTED: 1)
  int c0;             // XF_CLASS: the class of blockIdx.y = 0 (a launch covers at most 65535 classes)
  int cut_lds;        // the cutpoints a workgroup needs are staged in LDS behind the rows (LDS form)
};

// p_c = cdf_c - cdf_{c-1} with cdf_{-1} = 0 and cdf_{n_cut} = 1, the expression of k_score_store MODE 2 and k_accumulate_oprobit;
// lo / hi: cut[c - 1] / cut[c] (unused where has_lo / has_hi is false)
__device__ __forceinline__ double oprobit_cdf(double cut, double score) { return (1.0 + erf((cut - score) * 0.70710678118654752440)) / 2.0; }
__device__ __forceinline__ double oprobit_class_prob(double score, bool has_lo, double lo, bool has_hi, double hi) {
  const double prev = has_lo ? oprobit_cdf(lo, score) : 0.0;
  return has_hi ? oprobit_cdf(hi, score) - prev : 1.0 - prev;
}
// sum_{c = 1 .. n_cut} c p_c in ascending class order
__device__ __forceinline__ double oprobit_expected(double score, const double *cut, int n_cut) {
  double prev = 0.0, e = 0.0;
  for (int c = 0; c < n_cut; c++) {
    const double cdf = oprobit_cdf(cut[c], score);
    if (c > 0) e += (double)c * (cdf - prev);
    prev = cdf;
  }
  return e + (double)n_cut * (1.0 - prev);
}

// mean = (v_0 + v_1 + ...) * (1 / S), the sum and the factor of the predictors; the variance two-pass about the mean of
// the values shifted by v_0 (exactly 0 when all values are equal, and no cancellation against a large common offset)
template <class Get>
__device__ __forceinline__ void dist_moments(const Get &v, int S, double inv_S, double &mean, double &var) {
  const double v0 = v(0);
  double sum = v0, dsum = 0.0;
  for (int s = 1; s < S; s++) {
    const double x = v(s);
    sum += x;
    dsum += x - v0;
  }
  mean = sum * inv_S;
  const double md = dsum * inv_S;
  double ss = 0.0;
  for (int s = 0; s < S; s++) {
    const double e = (v(s) - v0) - md;
    ss += e * e;
  }
  var = ss * inv_S;
}

// y with mean_s Phi((y - v_s) sqa_s) = p: Newton steps kept inside a bracket that every evaluation shrinks, a bisection step
// wherever Newton leaves it (or the density underflows); at most DIST_SOLVE_STEPS evaluations, the last 140 of them plain
// bisection (which ends at neighbouring doubles). Ends after a Newton step below 1e-11 of the scale: the step after it
// (quadratic convergence) is below the evaluation's rounding.
constexpr int DIST_SOLVE_STEPS = 200;
__device__ __forceinline__ double dist_mixture_quantile(const double *v, const double *sqa, int S, double inv_S, double z, double p) {
  double lo = v[0] + z / sqa[0], hi = lo;
  for (int s = 1; s < S; s++) {
    const double y = v[s] + z / sqa[s];
    lo = fmin(lo, y);
    hi = fmax(hi, y);
  }
  if (!(lo < hi)) return lo;
  const double width = hi - lo;
  double y = 0.5 * (lo + hi);
  for (int it = 0; it < DIST_SOLVE_STEPS; it++) {
    double F = 0.0, f = 0.0;
    for (int s = 0; s < S; s++) {
      const double a = sqa[s];
      const double x = (y - v[s]) * a;
      F += 0.5 * erfc(-x * 0.70710678118654752440);
      f += a * exp(-0.5 * x * x);
    }
    F *= inv_S;
    f *= inv_S * 0.39894228040143267794;
    const double r = F - p;
    if (r == 0.0) break;
    if (r < 0.0)
      lo = y;
    else
      hi = y;
    double yn = y - r / f;
    const bool newton = it < DIST_SOLVE_STEPS - 140 && f > 0.0 && yn > lo && yn < hi;
    if (!newton) yn = 0.5 * (lo + hi);
    if (!(yn > lo && yn < hi)) break;  // lo and hi are neighbours
    const double step = fabs(yn - y);
    y = yn;
    if (newton && step <= 1e-11 * (fabs(y) + width)) break;
  }
  return y;
}

// One launch per row tile. LDS form (quantiles asked for): a workgroup brings R rows' S values into LDS (row stride odd: the
// row-per-lane phases are conflict-free), lane r computes row r's moments, then either all R rows are sorted in place by one
// bitonic network over P = S padded with +inf (every compare-exchange of a step spread over the workgroup) and thread (q, r)
// interpolates quantile q of row r as numpy's "linear" rule does, or (noise) thread (q, r) solves the mixture quantile with
// the row's scores and sqrt(alpha_s) read from LDS (the latter at one address for all lanes: a broadcast read).
// Direct form (LDS_ROWS = false, no quantiles, any S): a thread per row reads the scratch itself.
// XF (ordered probit, never with noise): the value of (sample s, row t) is a function of scratch[s][t] and cut[s][.], computed
// where the score leaves the scratch -- on the way into the sort buffer (the moments are taken from that buffer, there is no
// second one), or at the read of the direct form. XF_CLASS: blockIdx.y is the class; every class block reads the tile's scores
// again (from L2) and writes its outputs with stride C. The two cutpoints of every sample that a class needs (XF_EXPECTED: all
// n_cut) are staged in LDS behind the rows, where sqrt(alpha) goes with noise, if the launcher found room for them; else they
// are read from global memory (one address per sample for the whole workgroup).
// The identity takes RowSummaryArgs alone and the transforms RowTransformArgs after it (the pack X is empty or that one type), so
// that the identity's arguments, instructions and kernel descriptor are those of the kernel without transforms.
__device__ __forceinline__ RowTransformArgs row_transform_args() { return RowTransformArgs{}; }
__device__ __forceinline__ RowTransformArgs row_transform_args(const RowTransformArgs &x) { return x; }
template <bool LDS_ROWS, int XF = XF_NONE, class... X>
__global__ __launch_bounds__(WG) void k_row_summary(RowSummaryArgs a, X... xs) {
  static_assert(sizeof...(X) == (XF == XF_NONE ? 0 : 1), "a transform takes RowTransformArgs, the identity nothing");
  const RowTransformArgs x = row_transform_args(xs...);
  extern __shared__ double dist_lds[];
  const int S = a.S;
  const int c = XF == XF_CLASS ? x.c0 + (int)blockIdx.y : 0;
  const bool has_lo = c > 0, has_hi = c < x.n_cut;
  // output i of the identity is output i * C + c of the class form
  const auto at = [&](size_t i) { return XF == XF_CLASS ? i * (size_t)x.C + (size_t)c : i; };
  if (!LDS_ROWS) {
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (t >= a.Tn) return;
    const double *__restrict__ col = a.scratch + t;
    const int64_t Tn = a.Tn;
    double mean, var;
    if constexpr (XF == XF_NONE) {
      dist_moments([&](int s) { return col[(size_t)s * Tn]; }, S, a.inv_S, mean, var);
      a.mean[t] = mean;
      a.sd[t] = sqrt(var + a.noise_var);
    } else {
      const auto value = [&](int s) {
        const double *cs = x.cut + (size_t)s * x.n_cut;
        const double score = col[(size_t)s * Tn];
        if constexpr (XF == XF_CLASS)
          return oprobit_class_prob(score, has_lo, has_lo ? cs[c - 1] : 0.0, has_hi, has_hi ? cs[c] : 0.0);
        else
          return oprobit_expected(score, cs, x.n_cut);
      };
      dist_moments(value, S, a.inv_S, mean, var);
      a.mean[at((size_t)t)] = mean;
      a.sd[at((size_t)t)] = sqrt(var);
    }
    return;
  }
  const int R = a.R, st = a.stride, P = a.P;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(a.Tn - r0 < R ? a.Tn - r0 : R);
  const int tid = threadIdx.x;
  if constexpr (XF == XF_NONE) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      dist_lds[r * st + s] = r < nr ? a.scratch[(size_t)s * a.Tn + r0 + r] : 0.0;
    }
  } else {
    // the cutpoints of a value: XF_CLASS cut[s * cw + co - 1], cut[s * cw + co]; XF_EXPECTED cut[s * cw + 0 .. n_cut). (Called
    // once with the LDS pointer and once with the global one, so that neither becomes a flat access.)
    const auto fill = [&](const double *cut, int cw, int co) {
      for (int i = tid; i < S * R; i += WG) {
        const int s = i / R, r = i - s * R;
        double v = 0.0;
        if (r < nr) {
          const double score = a.scratch[(size_t)s * a.Tn + r0 + r];
          const double *cs = cut + (size_t)s * cw;
          if constexpr (XF == XF_CLASS)
            v = oprobit_class_prob(score, has_lo, has_lo ? cs[co - 1] : 0.0, has_hi, has_hi ? cs[co] : 0.0);
          else
            v = oprobit_expected(score, cs, x.n_cut);
        }
        dist_lds[r * st + s] = v;
      }
    };
    if (x.cut_lds) {
      double *staged = dist_lds + R * st;
      if constexpr (XF == XF_CLASS) {
        for (int s = tid; s < S; s += WG) {
          const double *cs = x.cut + (size_t)s * x.n_cut;
          staged[2 * s] = has_lo ? cs[c - 1] : 0.0;
          staged[2 * s + 1] = has_hi ? cs[c] : 0.0;
        }
      } else {
        for (int i = tid; i < S * x.n_cut; i += WG) staged[i] = x.cut[i];
      }
      __syncthreads();
      if constexpr (XF == XF_CLASS)
        fill(staged, 2, 1);
      else
        fill(staged, x.n_cut, 0);
    } else {
      fill(x.cut, x.n_cut, c);
    }
  }
  double *sqa = dist_lds + R * st;  // (noise) sqrt(alpha_s) behind the rows: every lane of the solve reads the same address
  if (XF != XF_NONE || !a.noise)
    for (int i = tid; i < (P - S) * R; i += WG) {
      const int s = i / R, r = i - s * R;
      dist_lds[r * st + S + s] = __builtin_inf();
    }
  else
    for (int s = tid; s < S; s += WG) sqa[s] = a.sqa[s];
  __syncthreads();
  if (tid < nr) {
    const double *row = dist_lds + tid * st;
    double mean, var;
    dist_moments([&](int s) { return row[s]; }, S, a.inv_S, mean, var);
    a.mean[at((size_t)(r0 + tid))] = mean;
    a.sd[at((size_t)(r0 + tid))] = sqrt(XF == XF_NONE ? var + a.noise_var : var);
  }
  if (XF == XF_NONE && a.noise) {
    for (int w = tid; w < a.n_q * R; w += WG) {
      const int q = w / R, r = w - q * R;
      if (r < nr) a.q[(size_t)q * a.ldq + r0 + r] = dist_mixture_quantile(dist_lds + r * st, sqa, S, a.inv_S, a.g[q], a.p[q]);
    }
    return;
  }
  __syncthreads();  // (the moments read the rows in sample order)
  const int half = P >> 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < R * half; idx += WG) {
        const int r = idx / half, c2 = idx - r * half;
        const int i = ((c2 & ~(j - 1)) << 1) | (c2 & (j - 1));
        double *row = dist_lds + r * st;
        const double x0 = row[i], y = row[i | j];
        if ((x0 > y) == ((i & k) == 0)) {
          row[i] = y;
          row[i | j] = x0;
        }
      }
      __syncthreads();
    }
  for (int w = tid; w < a.n_q * R; w += WG) {
    const int q = w / R, r = w - q * R;
    if (r >= nr) continue;
    const double *row = dist_lds + r * st;
    const int lo = a.lo[q], hi = lo + 1 < S ? lo + 1 : lo;
    const double x0 = row[lo], y = row[hi], g = a.g[q];
    const double d = y - x0;
    a.q[at((size_t)q * a.ldq + r0 + r)] = g >= 0.5 ? y - d * (1.0 - g) : x0 + d * g;  // (numpy's _lerp)
  }
}
// x: the load transform `xf` (XF_CLASS / XF_EXPECTED) and its cutpoints, or null (the values are the stored ones)
static void launch_row_summary(hipStream_t s, RowSummaryArgs &a, int xf = XF_NONE, RowTransformArgs *x = nullptr) {
  // XF_CLASS: the classes are grid.y, at most 65535 of them per launch
  const auto launch_classes = [&](auto kernel, unsigned blocks, size_t lds) {
    const int n_class = xf == XF_CLASS ? x->C : 1;
    for (x->c0 = 0; x->c0 < n_class; x->c0 += 65535)
      hipLaunchKernelGGL(kernel, dim3(blocks, (unsigned)std::min(65535, n_class - x->c0)), dim3(WG), lds, s, a, *x);
  };
  if (a.n_q == 0) {
    if (xf == XF_CLASS)
      launch_classes(k_row_summary<false, XF_CLASS, RowTransformArgs>, (unsigned)cdiv(a.Tn, WG), 0);
    else if (xf == XF_EXPECTED)
      launch_classes(k_row_summary<false, XF_EXPECTED, RowTransformArgs>, (unsigned)cdiv(a.Tn, WG), 0);
    else
      hipLaunchKernelGGL(k_row_summary<false>, dim3((unsigned)cdiv(a.Tn, WG)), dim3(WG), 0, s, a);
    return;
  }
  int P = 1;
  while (P < a.S) P <<= 1;
  a.P = a.noise ? a.S : P;
  a.stride = a.P | 1;
  // R rows of `stride` doubles, with noise S more for sqrt(alpha), within DIST_LDS_BYTES -- but never less than one row: one
  // row of S = 4096 takes 32 776 B, with noise 65 544 B, above the default limit of dynamic LDS (opted into once per device)
  const int aux = a.noise ? a.S : 0;
  const int fit = (DIST_LDS_BYTES / (int)sizeof(double) - aux) / a.stride;
  a.R = (int)std::min<int64_t>(std::max(1, std::min(DIST_MAX_ROWS, fit)), a.Tn);
  if (xf != XF_NONE) {
    // The rows are sized as without a transform. The cutpoints that a workgroup needs -- two per sample for a class, all n_cut
    // for the expected index -- are staged behind the rows where the DIST_LDS_BYTES still hold them, and read from global memory
    // where not (S = 4096: the one row is all the LDS there is).
    const int64_t want = (int64_t)a.S * (xf == XF_CLASS ? 2 : x->n_cut);
    x->cut_lds = (int64_t)a.R * a.stride + want <= DIST_LDS_BYTES / (int)sizeof(double);
    const size_t lds = ((size_t)a.R * a.stride + (x->cut_lds ? (size_t)want : 0)) * sizeof(double);  // <= 48 KB, or one row: 32 776 B
    if (xf == XF_CLASS)
      launch_classes(k_row_summary<true, XF_CLASS, RowTransformArgs>, (unsigned)cdiv(a.Tn, a.R), lds);
    else
      launch_classes(k_row_summary<true, XF_EXPECTED, RowTransformArgs>, (unsigned)cdiv(a.Tn, a.R), lds);
    return;
  }
  const size_t lds = ((size_t)a.R * a.stride + aux) * sizeof(double);
  static DeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {
    void (*const identity)(RowSummaryArgs) = k_row_summary<true>;
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)identity, hipFuncAttributeMaxDynamicSharedMemorySize, DIST_LDS_MAX_BYTES));
    raised.mark();
  }
  hipLaunchKernelGGL(k_row_summary<true>, dim3((unsigned)cdiv(a.Tn, a.R)), dim3(WG), lds, s, a);
}

// The tiled pass over the design that design_summary here, design_logdens (mfm_logdens.hpp) and design_loo (mfm_psis.hpp) share
// (DESIGN 4.9.1). Stage 1: the values of the rows [r0, r0 + Tn), all samples, into d->dist_scratch [S][Tn]. begin: once per call,
// behind the store's latest snapshot; designs without relation blocks (rank <= 512) stage their samples for the one-pass scorer,
// in chunks of `chunk` samples.
struct DistStage1 {
  bool one_pass;
  int chunk;
  int built;  // the chunk whose row-major V copies vt_all holds
};
static DistStage1 dist_stage1_begin(mfm_design *d, hipStream_t s, const SampleView &v, int32_t chunk_samples) {
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(s, v.pushed, 0));
  const bool one_pass = d->blocks.empty() && v.K <= 512;
  return DistStage1{one_pass, one_pass ? design_stage_samples(d, s, v, chunk_samples) : v.count(), -1};
}
// mode 0: scores, 1: Phi(score)
static void dist_stage1_tile(mfm_design *d, hipStream_t s, const SampleView &v, DistStage1 &st, int mode, int64_t r0, int64_t Tn) {
  const int count = v.count(), rank = v.K;
  const int64_t D = d->D;
  if (st.one_pass) {
    for (int c0 = 0; c0 < count; c0 += st.chunk) {
      const int C = std::min(st.chunk, count - c0);
      const ScoreStoreArgs sa = design_sample_chunk(d, s, c0, C, st.built != c0);
      st.built = c0;
      launch_score_store_rows(s, 3 + mode, d->X, score_rows(d->X, r0, Tn), sa, D, rank, d->KS, d->dist_scratch.p + (size_t)c0 * Tn);
    }
  } else {
    // relation blocks: the per-sample pass over the whole design, of which this tile's rows are kept (a design of more
    // than one tile is scored once per tile)
    for (int k = 0; k < count; k++) {
      const double *w = v.wv[(size_t)k], *V = w + D;
      score_design(s, d->timing, 1, d->X, d->blocks, D, rank, d->KS, v.w0[(size_t)k], w, V, d->Vt.p, nullptr, nullptr, d->score.p);
      hipLaunchKernelGGL(k_dist_copy, dim3((unsigned)cdiv(Tn, WG)), dim3(WG), 0, s, d->score.p + r0, d->dist_scratch.p + (size_t)k * Tn, Tn,
                         mode);
    }
  }
}

// The pass in its two steps, between which a caller uploads what its stage 2 reads (their order on the stream). reserve (N > 0): the
// rank's caches, the tile of T rows (tile_rows, or what DIST_SCRATCH_BYTES hold of all samples), room for it and for out_n outputs.
static int64_t dist_tiles_reserve(mfm_design *d, const SampleView &v, int64_t tile_rows, size_t out_n) {
  const int count = v.count();
  design_use_rank(d, v.K, d->stream);
  const int64_t T = std::min<int64_t>(d->N, tile_rows > 0 ? tile_rows : std::max<int64_t>(1, (int64_t)(DIST_SCRATCH_BYTES / sizeof(double)) / count));
  if (d->dist_scratch.n < (size_t)(T * count)) d->dist_scratch.alloc((size_t)(T * count));
  if (d->dist_out.n < out_n) d->dist_out.alloc(out_n);
  return T;
}
// `len` doubles of d->dist_out from `off` on, which leave for `host` when the last tile is done (len 0: nothing to copy)
struct DistColumn {
  double *host;
  size_t off, len;
};
// run: per tile stage 1 in `mode`, then stage2(r0, Tn), the caller's launch over the scratch; out_sn, where not null: the host's
// (S, N) matrix, whose columns r0 .. r0 + Tn are what stage 2 left in the scratch [S][Tn]. Then the columns go back, and one wait.
template <class Stage2>
static void dist_tiles_run(mfm_design *d, const SampleView &v, int64_t T, int mode, int32_t chunk_samples, double *out_sn,
                           std::initializer_list<DistColumn> columns, const Stage2 &stage2) {
  hipStream_t s = d->stream;
  const int64_t N = d->N;
  DistStage1 st = dist_stage1_begin(d, s, v, chunk_samples);
  for (int64_t r0 = 0; r0 < N; r0 += T) {
    const int64_t Tn = std::min<int64_t>(T, N - r0);
    dist_stage1_tile(d, s, v, st, mode, r0, Tn);
    MFM_HIP_CHECK(hipGetLastError());
    stage2(r0, Tn);
    MFM_HIP_CHECK(hipGetLastError());
    if (out_sn)
      MFM_HIP_CHECK(hipMemcpy2DAsync(out_sn + r0, (size_t)N * sizeof(double), d->dist_scratch.p, (size_t)Tn * sizeof(double),
                                     (size_t)Tn * sizeof(double), (size_t)v.count(), hipMemcpyDeviceToHost, s));
  }
  for (const DistColumn &c : columns)
    if (c.len) MFM_HIP_CHECK(hipMemcpyAsync(c.host, d->dist_out.p + c.off, c.len * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

// The argument checks that the summaries and the log densities (logdens_check, mfm_logdens.hpp) share; nothing here touches the device.
static void check_tiling(int64_t tile_rows, int32_t chunk_samples) {
  if (tile_rows < 0 || chunk_samples < 0) throw Error(MFM_ERR_INVALID, "negative tiling override");
}
static void check_precisions(const double *p, int count) {
  for (int k = 0; k < count; k++)
    if (!(p[k] > 0.0) || !std::isfinite(p[k])) throw Error(MFM_ERR_INVALID, "noise precisions must be positive and finite");
}
static void check_cutpoints(const double *c, int count, int n_cut) {
  for (int k = 0; k < count; k++)
    for (int j = 0; j < n_cut; j++) {
      const double *cs = c + (size_t)k * n_cut;
      if (!std::isfinite(cs[j]) || (j > 0 && !(cs[j - 1] <= cs[j])))
        throw Error(MFM_ERR_INVALID, "cutpoints must be finite and ascending within every sample");
    }
}

// what an ordered-probit summary adds to the call: which value, and the samples' cutpoints [count][n_cut] on the host
struct OprobitValues {
  int32_t expected, n_cut;
  const double *cutpoints;
};

// op: summarise class probabilities / the expected class index of the scores (mode 0) instead of the scores; the outputs then
// hold C = n_cut + 1 (expected: 1) values per row, row-major (N, C) and (n_q, N, C)
static void design_summary(mfm_design *d, const SampleView &v, int32_t mode, int32_t n_q, const double *probs, const double *precisions,
                           const double *z, int64_t tile_rows, int32_t chunk_samples, double *out_mean, double *out_std, double *out_q,
                           const OprobitValues *op = nullptr) {
  const int count = v.count();
  check_sample_source(d, v);
  if (mode < 0 || mode > 1) throw Error(MFM_ERR_INVALID, "bad summary mode (0: score, 1: Phi(score))");
  if (n_q < 0 || n_q > DIST_MAX_Q) throw Error(MFM_ERR_INVALID, "at most " + std::to_string(DIST_MAX_Q) + " quantiles per call");
  if (n_q > 0 && count > DIST_MAX_S)
    throw Error(MFM_ERR_INVALID, "quantiles are computed over at most " + std::to_string(DIST_MAX_S) + " samples, got " + std::to_string(count));
  if (n_q > 0 && !probs) throw Error(MFM_ERR_INVALID, "quantiles asked for without their probabilities");
  if (precisions && mode != 0) throw Error(MFM_ERR_INVALID, "noise precisions apply to scores (mode 0) only");
  if (precisions && n_q > 0 && !z) throw Error(MFM_ERR_INVALID, "noise quantiles need Phi^-1 of their probabilities");
  check_tiling(tile_rows, chunk_samples);
  for (int q = 0; q < n_q; q++) {
    const bool inside = precisions ? probs[q] > 0.0 && probs[q] < 1.0 && std::isfinite(z[q]) : probs[q] >= 0.0 && probs[q] <= 1.0;
    if (!inside) throw Error(MFM_ERR_INVALID, "quantile probability out of range ([0, 1]; with noise strictly inside)");
  }
  if (precisions) check_precisions(precisions, count);
  if (op) {
    if (op->expected < 0 || op->expected > 1) throw Error(MFM_ERR_INVALID, "bad value selector (0: class probabilities, 1: expected class index)");
    if (op->n_cut < 1) throw Error(MFM_ERR_INVALID, "an ordered-probit summary needs at least one cutpoint per sample");
    if (!op->cutpoints) throw Error(MFM_ERR_INVALID, "an ordered-probit summary needs the samples' cutpoints");
    check_cutpoints(op->cutpoints, count, op->n_cut);
  }
  const int xf = !op ? XF_NONE : op->expected ? XF_EXPECTED : XF_CLASS;
  const int64_t C = xf == XF_CLASS ? (int64_t)op->n_cut + 1 : 1;
  hipStream_t s = d->stream;
  const int64_t N = d->N;
  if (N == 0) return;
  const size_t NC = (size_t)N * (size_t)C;
  const int64_t T = dist_tiles_reserve(d, v, tile_rows, NC * (2 + n_q));
  RowSummaryArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scratch = d->dist_scratch.p;
  a.ldq = N;
  a.S = count;
  a.n_q = n_q;
  a.noise = precisions != nullptr;
  a.inv_S = 1.0 / count;
  if (precisions) {
    std::vector<double> sq((size_t)count);
    double nv = 0.0;
    for (int k = 0; k < count; k++) {
      sq[k] = std::sqrt(precisions[k]);
      nv += 1.0 / precisions[k];
    }
    a.noise_var = nv * a.inv_S;
    if (d->dist_aux.n < (size_t)count) d->dist_aux.alloc((size_t)count);
    MFM_HIP_CHECK(hipMemcpy(d->dist_aux.p, sq.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    a.sqa = d->dist_aux.p;
  }
  RowTransformArgs x{};
  if (op) {
    const size_t n = (size_t)count * op->n_cut;
    if (d->cut.n < n) d->cut.alloc(n);
    MFM_HIP_CHECK(hipMemcpyAsync(d->cut.p, op->cutpoints, n * sizeof(double), hipMemcpyHostToDevice, s));
    x.cut = d->cut.p;
    x.n_cut = op->n_cut;
    x.C = (int)C;
  }
  for (int q = 0; q < n_q; q++) {
    a.p[q] = probs[q];
    if (precisions) {
      a.g[q] = z[q];
    } else {  // numpy's "linear" rule: position (S - 1) p between the order statistics floor and floor + 1
      const double h = (double)(count - 1) * probs[q];
      const double fl = std::floor(h);
      a.lo[q] = (int)std::min<double>(fl, (double)(count - 1));
      a.g[q] = h - fl;
    }
  }
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    a.Tn = Tn;
    a.mean = d->dist_out.p + (size_t)r0 * C;
    a.sd = d->dist_out.p + NC + (size_t)r0 * C;
    a.q = d->dist_out.p + 2 * NC + (size_t)r0 * C;
    launch_row_summary(s, a, xf, &x);
  };
  dist_tiles_run(d, v, T, mode, chunk_samples, nullptr, {{out_mean, 0, NC}, {out_std, NC, NC}, {out_q, 2 * NC, NC * n_q}}, stage2);
}

}  // namespace mfm

extern "C" {

int mfm_design_summary_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t n_q,
                             const double *probs, const double *precisions, const double *z, int64_t tile_rows,
                             int32_t chunk_samples, double *out_mean, double *out_std, double *out_q) {
  MFM_TRY(d)
  design_summary(d, samples_of_store(st, first, count), mode, n_q, probs, precisions, z, tile_rows, chunk_samples, out_mean, out_std, out_q);
  MFM_CATCH(d)
}

// host samples: all S uploaded for this call, then as above (the same kernels over the same chunks). Like a store's reservation
// the upload is refused beyond MFM_STORE_MAX_FRACTION of the free device memory, where mfm_design_predict, which streams one
// sample at a time, still runs.
int mfm_design_summary(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t mode, int32_t n_q, const double *probs, const double *precisions, const double *z,
                       int64_t tile_rows, int32_t chunk_samples, double *out_mean, double *out_std, double *out_q) {
  MFM_TRY(d)
  store_check_fraction(d->D, rank, n_samples);
  design_summary(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), mode, n_q, probs, precisions, z, tile_rows,
                 chunk_samples, out_mean, out_std, out_q);
  MFM_CATCH(d)
}

// ordered probit: the class probabilities (expected = 0; outputs (N, C), (N, C), (n_q, N, C) with C = n_cut + 1) or the expected
// class index (expected = 1; (N), (N), (n_q, N)) of every sample's score under that sample's cutpoints [count][n_cut]
int mfm_design_summary_oprobit_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t expected, int32_t n_cut,
                                     const double *cutpoints, int32_t n_q, const double *probs, int64_t tile_rows,
                                     int32_t chunk_samples, double *out_mean, double *out_std, double *out_q) {
  MFM_TRY(d)
  const OprobitValues op{expected, n_cut, cutpoints};
  design_summary(d, samples_of_store(st, first, count), 0, n_q, probs, nullptr, nullptr, tile_rows, chunk_samples, out_mean, out_std, out_q, &op);
  MFM_CATCH(d)
}

int mfm_design_summary_oprobit(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                               int32_t expected, int32_t n_cut, const double *cutpoints, int32_t n_q, const double *probs,
                               int64_t tile_rows, int32_t chunk_samples, double *out_mean, double *out_std, double *out_q) {
  MFM_TRY(d)
  store_check_fraction(d->D, rank, n_samples);
  const OprobitValues op{expected, n_cut, cutpoints};
  design_summary(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), 0, n_q, probs, nullptr, nullptr, tile_rows,
                 chunk_samples, out_mean, out_std, out_q, &op);
  MFM_CATCH(d)
}

}  // extern "C"
