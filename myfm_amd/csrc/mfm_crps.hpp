// mfm_crps.hpp -- continuous ranked probability score over the kept samples (not in the reference): per test row the
// energy form CRPS = E|Y - y| - E|Y - Y'| / 2 of the posterior predictive distribution of y, Y and Y' independent draws of it, as
// its three pieces accuracy = E|Y - y|, spread = E|Y - Y'| / 2 and crps. Included by mfm_hip.hip after mfm_logdens.hpp.
//   regression      Y ~ (1 / S) sum_s N(score_s, v_s), v_s = 1 / alpha_s (the mixture of predict_dist(noise = True)); with
//                   A(m, v) = E|N(m, v)| = m erf(m h) + g exp(-(m h)^2), h = 1 / sqrt(2 v), g = sqrt(2 v / pi) (Grimit et al. 2006):
//                   accuracy = (1 / S) sum_s A(y - score_s, v_s),
//                   spread = (1 / S^2) sum_s [sum_{t < s} A(score_s - score_t, v_s + v_t) + g(2 v_s) / 2]   (A(0, v) = g)
//                   crps = accuracy - spread (>= (1 - 1 / sqrt 2) accuracy: the difference does not cancel)
//   classification, ordered probit   Y is the class index 0 .. n_cut (a classifier: n_cut = 1, the one cutpoint 0). Per cut j,
//                   d_j = |mean_s Phi(cut_sj - score_s) - 1[y <= j]|, the mean taken of the side that is small where d_j is:
//                   accuracy = sum_j d_j, spread = sum_j d_j (1 - d_j), crps = sum_j d_j^2 (summed itself, not a difference)
//
// Rows are processed by the tiled pass of mfm_dist.hpp (dist_tiles_run) in mode 0; the stage 2 given to it here is k_row_crps_mix
// or k_row_crps_cdf. Everything is fp64, there are no atomics, every sum runs in a fixed order (sample order inside, then the
// outer index in order): a rerun, another row tile or another sample chunk give the same bits.
#pragma once

namespace mfm {

constexpr int CRPS_MAX_S = 1024;  // samples per regression call: S (S + 1) / 2 pair terms per row, a table of S (S + 1) doubles
constexpr int CRPS_BLOCK = 4;     // samples whose pair sums a lane of k_row_crps_mix holds in registers (the listing)

// (h, g) of A(., v): h = 1 / sqrt(2 v), g = sqrt(2 v / pi). The pair (s, t) takes v = v_s + v_t, the accuracy term v = v_s.
__host__ __device__ __forceinline__ void crps_constants(double v, double &h, double &g) {
  const double v2 = 2.0 * v;
  h = 1.0 / sqrt(v2);
  g = sqrt(v2 / 3.14159265358979323846);
}
// A(m, v) = E|N(m, v)| from (h, g) of v; m h large: erf = +-1 and the exp term 0, A = |m|
__host__ __device__ __forceinline__ double crps_abs_normal(double m, double h, double g) {
  const double z = m * h;
  return m * erf(z) + g * exp(-(z * z));
}
// One sample's term of d_j with t = cut_sj - score_s: Phi(t) where the target lies above cut j (1[y <= j] = 0), else
// 1 - Phi(t) = Phi(-t); erfc of the signed argument, so a small d keeps its relative accuracy
__host__ __device__ __forceinline__ double crps_cdf_side(bool above, double t) {
  return 0.5 * erfc((above ? -t : t) * 0.70710678118654752440);
}

// The constants of a regression call, on the host once per call: (h, g) of v_s for s < S, then the triangular table of (h, g) of
// v_s + v_t at pair index s (s + 1) / 2 + t, t <= s. 2 S + S (S + 1) doubles.
static size_t crps_table_size(int S) { return 2 * (size_t)S + (size_t)S * ((size_t)S + 1); }
static void crps_table_fill(const double *precisions, int S, double *out) {
  double *tab = out + 2 * (size_t)S;
  for (int s = 0; s < S; s++) {
    const double vs = 1.0 / precisions[s];
    crps_constants(vs, out[2 * (size_t)s], out[2 * (size_t)s + 1]);
    double *row = tab + (size_t)s * ((size_t)s + 1);
    for (int t = 0; t <= s; t++) crps_constants(vs + 1.0 / precisions[t], row[2 * (size_t)t], row[2 * (size_t)t + 1]);
  }
}

struct RowCrpsArgs {
  const double *scratch;  // [S][Tn] the tile's scores
  const double *y;        // of the tile's first row
  const double *aux;      // regression: crps_table_fill's constants; ordered probit: cut[S][n_cut]
  double *crps, *accuracy, *spread;  // of the tile's first row
  int64_t Tn;
  int S, n_cut;
  int aux_lds;            // (ordered probit) the cutpoints are staged in LDS (they fit LOGDENS_LDS_BYTES)
  double inv_S;
};

// Stage 2 for regression, one launch per row tile: a thread per row, so consecutive lanes read consecutive scratch[s][t] and the
// pair (s, u) is the same for all lanes of a wavefront: its (h, g) is read at a wave-uniform address (scalar loads, no VALU). The
// s axis is blocked in registers: a lane holds the scores of B samples and their pair sums, and streams u = 0 .. s - 1 from the
// scratch once per block -- about S / (2 B) reads of the scratch per row, no LDS. The diagonal block and the last, partial block
// run the same loop text under wave-uniform conditions; the accuracy terms are a loop of their own in front. Pair sum s adds
// its terms in u order, the pair sums are added in s order: a row's result depends on neither the tiling nor B.
template <int B>
__global__ __launch_bounds__(WG) void k_row_crps_mix(RowCrpsArgs a) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= a.Tn) return;
  const int S = a.S;
  const int64_t Tn = a.Tn;
  const double *__restrict__ col = a.scratch + t;
  const double *__restrict__ own = a.aux;                  // (h, g) of v_s
  const double *__restrict__ tab = a.aux + 2 * (size_t)S;  // (h, g) of v_s + v_u
  const double yt = a.y[t];
  double acc = 0.0, total = 0.0;
  for (int s = 0; s < S; s++) acc += crps_abs_normal(yt - col[(size_t)s * Tn], own[2 * s], own[2 * s + 1]);
  for (int s0 = 0; s0 < S; s0 += B) {
    double mu[B], p[B];
#pragma unroll
    for (int i = 0; i < B; i++) {
      mu[i] = s0 + i < S ? col[(size_t)(s0 + i) * Tn] : 0.0;
      p[i] = 0.0;
    }
    const int u_end = (s0 + B < S ? s0 + B : S) - 1;  // the block's last sample pairs with u < u_end
    const int pair0 = s0 * (s0 + 1) / 2;              // of (s0, 0); row s + 1 of the table begins s + 1 entries behind row s
    for (int u = 0; u < u_end; u++) {
      const double mu_u = col[(size_t)u * Tn];
      int pair = pair0 + u;
#pragma unroll
      for (int i = 0; i < B; i++) {
        const int s = s0 + i;
        if (u < s && s < S) p[i] += crps_abs_normal(mu[i] - mu_u, tab[2 * pair], tab[2 * pair + 1]);
        pair += s + 1;
      }
    }
    int diag = pair0 + s0;  // of (s0, s0)
#pragma unroll
    for (int i = 0; i < B; i++) {
      const int s = s0 + i;
      if (s < S) {
        p[i] += 0.5 * tab[2 * diag + 1];
        total += p[i];
      }
      diag += s + 2;
    }
  }
  const double accuracy = acc * a.inv_S, spread = (total * a.inv_S) * a.inv_S;
  a.accuracy[t] = accuracy;
  a.spread[t] = spread;
  a.crps[t] = accuracy - spread;
}

// Stage 2 for classification and ordered probit, one launch per row tile: a thread per row, the loop over the cuts outside the
// loop over the samples (the tile's scores are read n_cut times, from L2). The cutpoints are read from LDS, staged once per
// workgroup, or -- where they do not fit -- from global memory at one address per (sample, cut) for the whole workgroup, as
// k_row_logdens reads them.
template <int TASK>
__global__ __launch_bounds__(WG) void k_row_crps_cdf(RowCrpsArgs a) {
  extern __shared__ double crps_lds[];
  const int S = a.S, n_cut = a.n_cut;
  const bool staged = TASK == LOGDENS_ORDERED && a.aux_lds;
  if (staged) {
    for (int i = threadIdx.x; i < S * n_cut; i += WG) crps_lds[i] = a.aux[i];
    __syncthreads();
  }
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= a.Tn) return;
  const int64_t Tn = a.Tn;
  const double *__restrict__ col = a.scratch + t;
  const double yt = a.y[t];
  // (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto run = [&](const double *cut) {
    double accuracy = 0.0, spread = 0.0, crps = 0.0;
    for (int j = 0; j < n_cut; j++) {
      const bool above = yt > (double)j;
      double d = 0.0;
      for (int s = 0; s < S; s++) {
        const double c = TASK == LOGDENS_ORDERED ? cut[(size_t)s * n_cut + j] : 0.0;
        d += crps_cdf_side(above, c - col[(size_t)s * Tn]);
      }
      d *= a.inv_S;
      accuracy += d;
      spread += d * (1.0 - d);
      crps += d * d;
    }
    a.accuracy[t] = accuracy;
    a.spread[t] = spread;
    a.crps[t] = crps;
  };
  if (staged)
    run(crps_lds);
  else
    run(a.aux);
}

static void launch_row_crps(hipStream_t s, int task, const RowCrpsArgs &a) {
  const dim3 grid((unsigned)cdiv(a.Tn, WG));
  if (task == LOGDENS_REGRESSION) {
    hipLaunchKernelGGL(k_row_crps_mix<CRPS_BLOCK>, grid, dim3(WG), 0, s, a);
  } else if (task == LOGDENS_CLASSIFICATION) {
    hipLaunchKernelGGL(k_row_crps_cdf<LOGDENS_CLASSIFICATION>, grid, dim3(WG), 0, s, a);
  } else {
    const size_t lds = a.aux_lds ? (size_t)a.S * a.n_cut * sizeof(double) : 0;
    hipLaunchKernelGGL(k_row_crps_cdf<LOGDENS_ORDERED>, grid, dim3(WG), lds, s, a);
  }
}

// One row on the host by the functions and in the orders of the two kernels: out = (crps, accuracy, spread). aux: crps_table_fill's
// constants (regression); cut[S][n_cut] (ordered probit).
static void crps_row_host(int task, int S, double y, const double *scores, const double *aux, int n_cut, const double *cut, double *out) {
  const double inv_S = 1.0 / S;
  if (task == LOGDENS_REGRESSION) {
    const double *tab = aux + 2 * (size_t)S;
    double acc = 0.0, total = 0.0;
    for (int s = 0; s < S; s++) {
      acc += crps_abs_normal(y - scores[s], aux[2 * (size_t)s], aux[2 * (size_t)s + 1]);
      const double *row = tab + (size_t)s * ((size_t)s + 1);
      double p = 0.0;
      for (int u = 0; u < s; u++) p += crps_abs_normal(scores[s] - scores[u], row[2 * (size_t)u], row[2 * (size_t)u + 1]);
      p += 0.5 * row[2 * (size_t)s + 1];
      total += p;
    }
    out[1] = acc * inv_S;
    out[2] = (total * inv_S) * inv_S;
    out[0] = out[1] - out[2];
    return;
  }
  double accuracy = 0.0, spread = 0.0, crps = 0.0;
  for (int j = 0; j < n_cut; j++) {
    const bool above = y > (double)j;
    double d = 0.0;
    for (int s = 0; s < S; s++) d += crps_cdf_side(above, (task == LOGDENS_ORDERED ? cut[(size_t)s * n_cut + j] : 0.0) - scores[s]);
    d *= inv_S;
    accuracy += d;
    spread += d * (1.0 - d);
    crps += d * d;
  }
  out[0] = crps;
  out[1] = accuracy;
  out[2] = spread;
}

// Every argument check of a call over `count` samples and N rows: those of a log density (logdens_check, the three outputs in the
// place of its three), and for regression the sample limit. Nothing here touches the device.
static void crps_check(const LogdensCall &c, int64_t N, int count) {
  logdens_check(c, N, count);
  if (c.task == LOGDENS_REGRESSION && count > CRPS_MAX_S)
    throw Error(MFM_ERR_INVALID, "a regression CRPS is computed over at most " + std::to_string(CRPS_MAX_S) + " samples, got " + std::to_string(count));
}

static void design_crps(mfm_design *d, const SampleView &v, const LogdensCall &c) {
  const int count = v.count();
  check_sample_source(d, v);
  hipStream_t s = d->stream;
  const size_t N = (size_t)d->N;
  if (N == 0) return;
  const int64_t T = dist_tiles_reserve(d, v, c.tile_rows, N * 3);  // crps, accuracy, spread
  RowCrpsArgs a;
  std::memset(&a, 0, sizeof(a));
  if (c.task == LOGDENS_REGRESSION) {
    // the targets as logdens_upload sends them; the constants are this file's own
    if (d->dist_y.n < N) d->dist_y.alloc(N);
    MFM_HIP_CHECK(hipMemcpyAsync(d->dist_y.p, c.y, N * sizeof(double), hipMemcpyHostToDevice, s));
    const size_t n_aux = crps_table_size(count);
    std::vector<double> aux(n_aux);
    crps_table_fill(c.precisions, count, aux.data());
    if (d->dist_aux.n < n_aux) d->dist_aux.alloc(n_aux);
    MFM_HIP_CHECK(hipMemcpy(d->dist_aux.p, aux.data(), n_aux * sizeof(double), hipMemcpyHostToDevice));
    a.aux = d->dist_aux.p;
  } else {
    const LogdensConstants k = logdens_upload(d, s, c, d->N, count);
    a.aux = k.aux;
    a.aux_lds = k.n_aux > 0 && k.n_aux * sizeof(double) <= (size_t)LOGDENS_LDS_BYTES;
  }
  a.scratch = d->dist_scratch.p;
  a.S = count;
  a.inv_S = 1.0 / count;
  a.n_cut = c.task == LOGDENS_ORDERED ? c.n_cut : 1;  // (a classifier: the one cutpoint 0)
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    a.Tn = Tn;
    a.y = d->dist_y.p + r0;
    a.crps = d->dist_out.p + r0;
    a.accuracy = d->dist_out.p + N + r0;
    a.spread = d->dist_out.p + 2 * N + r0;
    launch_row_crps(s, c.task, a);
  };
  dist_tiles_run(d, v, T, 0, c.chunk_samples, nullptr, {{c.out_lpd, 0, N}, {c.out_mean, N, N}, {c.out_var, 2 * N, N}}, stage2);
}

// the call of a CRPS in the words of a log density: its three outputs stand where lpd, mean and var do
static LogdensCall crps_call(int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                             int64_t tile_rows, int32_t chunk_samples, double *out_crps, double *out_accuracy, double *out_spread) {
  return LogdensCall{task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_crps, out_accuracy, out_spread, nullptr, nullptr};
}

}  // namespace mfm

extern "C" {

int mfm_design_crps_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                          const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                          double *out_crps, double *out_accuracy, double *out_spread) {
  MFM_TRY(d)
  const LogdensCall c = crps_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_crps, out_accuracy, out_spread);
  crps_check(c, d->N, std::max(count, 0));
  design_crps(d, samples_of_store(st, first, count), c);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_crps(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t task,
                    const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                    int32_t chunk_samples, double *out_crps, double *out_accuracy, double *out_spread) {
  MFM_TRY(d)
  const LogdensCall c = crps_call(task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out_crps, out_accuracy, out_spread);
  crps_check(c, d->N, std::max(n_samples, 0));
  store_check_fraction(d->D, rank, n_samples);
  design_crps(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), c);
  MFM_CATCH(d)
}

// one row on the host, by the functions the kernels run and in their summation orders: out = (crps, accuracy, spread)
int mfm_crps_row(int32_t task, int32_t S, double y, const double *scores, const double *precisions, int32_t n_cut, const double *cutpoints,
                 double *out) {
  try {
    if (S < 1 || !scores || !out) throw mfm::Error(MFM_ERR_INVALID, "a row of at least one score and the output of three values are needed");
    mfm::crps_check(mfm::crps_call(task, &y, precisions, n_cut, cutpoints, 0, 0, out, out + 1, out + 2), 1, S);
    for (int s = 0; s < S; s++)
      if (!std::isfinite(scores[s])) throw mfm::Error(MFM_ERR_INVALID, "scores must be finite");
    std::vector<double> aux;
    if (task == mfm::LOGDENS_REGRESSION) {
      aux.resize(mfm::crps_table_size(S));
      mfm::crps_table_fill(precisions, S, aux.data());
    }
    mfm::crps_row_host(task, S, y, scores, aux.data(), task == mfm::LOGDENS_ORDERED ? n_cut : 1, cutpoints, out);
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
