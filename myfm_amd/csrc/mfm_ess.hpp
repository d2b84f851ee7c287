// mfm_ess.hpp -- convergence diagnostics of the kept samples, per row of the design (not in the reference): split
// R-hat, bulk and mean effective sample size and the Monte Carlo standard error after Vehtari, Gelman, Simpson, Carpenter and
// Buerkner (2021), of the value that predict_dist summarises (kind 0) or of the likelihood that predict_loo weights by (kind 1:
// u_s = exp(l_s - max_s l_s), the relative efficiency r_eff = ess / S and the delta-method error of lpd). Included by mfm_hip.hip
// after mfm_psis.hpp.
//
// The tiled pass is that of mfm_dist.hpp (dist_tiles_run, mode 0: the scores of a row tile, sample-major, in the scratch); its
// stage 2 here, k_row_ess, follows the LDS form of k_row_psis. Everything is fp64, there are no atomics; every sum over samples
// runs in sample order and every sum over lags in lag order, so a row's result depends on its own samples alone: another row
// tile, sample chunk, number of rows per workgroup or a rerun give the same bits. mfm_ess_row runs one sequence on the host
// through the same scalar pieces in the same orders.
//
// Several chains: the S samples may be M chains of L = S / M draws each, chain after chain (n_chains of the *_chains entries). Each
// chain is split as one chain is, n = L / 2: sequence 2m is x[mL .. mL + n), sequence 2m + 1 is x[mL + L - n .. mL + L), C = 2M
// sequences in all; ranks, the median, the mean and the standard deviation are taken over all S draws. With M = 1 every operation
// below is the one the single-chain form made, in its order: the same bits.
#pragma once
#include <algorithm>
#include <numeric>

#include "mfm_normal_quantile.hpp"

namespace mfm {

constexpr int ESS_MIN_HALF = 4;      // a half of fewer draws (a chain of L < 8) is not diagnosed: NaN
constexpr int ESS_MAX_CHAINS = 32;   // 2 x 32 sequences: a lane of the row's wavefront per sequence
constexpr int ESS_MAX_ROWS = 32;     // rows per workgroup
constexpr int ESS_LDS_BYTES = 64 * 1024;       // per workgroup, where more than one row fits
constexpr int ESS_LDS_MAX_BYTES = 160 * 1024;  // what a workgroup of gfx950 can have: one row of DIST_MAX_S samples takes 114 784 B
constexpr int ESS_HDR = 9;           // doubles of a row's header (odd, like the row strides)
constexpr int ESS_H_MAX = 0, ESS_H_MID_LO = 1, ESS_H_T = 2, ESS_H_R = 3, ESS_H_ESS_MEAN = 4, ESS_H_ESS_BULK = 5, ESS_H_R_BULK = 6, ESS_H_MID_HI = 7;

// ---- the scalar pieces, host and device ----------------------------------------------------------------------------------------
// d_i = x_i - mu_h, taken about the half's first draw x_0: with m = (sum_i (x_i - x_0)) / n it is (x_i - x_0) - m and mu_h = x_0 + m.
// A half of equal values has d = 0 exactly, whatever the value (the sum of n copies of 0.1, divided by n, is not 0.1), and values
// that lie close together keep their digits.
__host__ __device__ __forceinline__ double ess_centered(double x, double x0, double m) { return (x - x0) - m; }
// A(t) from the C sequences' sums of d_i d_{i+t}: the mean of the biased autocovariances c_h(t) = sum / n, added up in sequence
// order, a chain's two halves at a time (acc starts at 0) ...
__host__ __device__ __forceinline__ double ess_autocov_add(double acc, double sum_a, double sum_b, int n) {
  return (acc + sum_a / (double)n) + sum_b / (double)n;
}
__host__ __device__ __forceinline__ double ess_autocov_mean(double acc, int C) { return acc / (double)C; }
// ... of which one chain is the case C = 2, written out
__host__ __device__ __forceinline__ double ess_autocov(double sum_a, double sum_b, int n) {
  return (sum_a / (double)n + sum_b / (double)n) / 2.0;
}
// W = A(0) n / (n - 1), V = A(0) + B with B the variance (ddof = 1) of the C sequences' means mean_of(c) about their mean, both sums
// in sequence order
__host__ __device__ __forceinline__ double ess_within(double A0, int n) { return A0 * (double)n / (double)(n - 1); }
template <class MeanOf>
__host__ __device__ __forceinline__ double ess_total(double A0, int C, const MeanOf &mean_of) {
  double g = mean_of(0);
  for (int c = 1; c < C; c++) g += mean_of(c);
  g /= (double)C;
  double B = (mean_of(0) - g) * (mean_of(0) - g);
  for (int c = 1; c < C; c++) B += (mean_of(c) - g) * (mean_of(c) - g);
  return A0 + B / (double)(C - 1);
}
__host__ __device__ __forceinline__ double ess_total(double A0, double mu_a, double mu_b) {  // (C = 2, written out)
  const double g = (mu_a + mu_b) / 2.0;
  return A0 + ((mu_a - g) * (mu_a - g) + (mu_b - g) * (mu_b - g));
}
// sequence c of a row of M chains of L draws, n = L / 2: where it starts
__host__ __device__ __forceinline__ int ess_sequence_start(int c, int L, int n) { return (c >> 1) * L + ((c & 1) ? L - n : 0); }
// no diagnosis: W is not > 0 (a constant half-pair) or not finite (a non-finite draw)
__host__ __device__ __forceinline__ bool ess_within_ok(double W) { return W > 0.0 && W < __builtin_inf(); }
__host__ __device__ __forceinline__ double ess_rho(double W, double A, double V) { return 1.0 - (W - A) / V; }
// Geyer's initial positive sequence as Stan runs it: the loop goes on, and a pair is kept
__host__ __device__ __forceinline__ bool ess_geyer_continue(int t, int n, double re, double ro) { return t < n - 5 && re + ro > 0.0; }
__host__ __device__ __forceinline__ bool ess_geyer_keep(double re, double ro) { return re + ro >= 0.0; }
// the floor of tau: ess <= draws log10(draws), draws = C n the draws that the sequences hold
__host__ __device__ __forceinline__ double ess_tau_floor(int draws) { return 1.0 / log10((double)draws); }
// the tie group at the sorted positions first .. last (0-based) has the average rank r = ((first + 1) + (last + 1)) / 2, a
// multiple of 1/2: its z is table[2r - 2]
__host__ __device__ __forceinline__ int ess_tie_table_index(int first, int last) { return first + last; }
// |x - med| with numpy's "linear" median of S ascending values (k_row_summary's interpolation at p = 0.5), from the order statistics
// lo = x[(S - 1) / 2] and hi = x[S / 2] between which it lies: every draw is <= lo or >= hi, and its distance to med = (lo + hi) / 2
// is its distance to that neighbour plus h = (hi - lo) / 2. Odd S: lo = hi = med, h = 0, the plain difference. Even S: the two
// middle draws are equally far from the median, and this form gives them equal values, h, in floating point as well -- the
// rounded |x - med| makes them a tie or not by the last bit of the draws, and a rank apart in Z.
__host__ __device__ __forceinline__ double ess_folded(double x, double lo, double hi) {
  const double h = (hi - lo) * 0.5;
  return x >= hi ? (x - hi) + h : (lo - x) + h;
}

// Geyer's first loop, resumable: the lags [0, avail) are known (A(t) gives them), put(t, rho) stores an entry of the sequence.
// Returns false when it needs lags from avail on (the next batch), true when it has truncated: T = g.t. The entries below T are
// all stored; of the last pair rho[T] is stored (0 where the pair was not kept) and rho[T + 1], which nothing reads, is not.
struct EssGeyer {
  int t;
  double re, ro;
};
template <class GetA, class PutRho>
__host__ __device__ __forceinline__ bool ess_geyer_advance(EssGeyer &g, int n, int avail, double W, double V, const GetA &A,
                                                           const PutRho &put) {
  while (ess_geyer_continue(g.t, n, g.re, g.ro)) {
    if (g.t + 3 >= avail) return false;
    g.t += 2;
    g.re = ess_rho(W, A(g.t), V);
    g.ro = ess_rho(W, A(g.t + 1), V);
    if (ess_geyer_keep(g.re, g.ro)) {
      put(g.t, g.re);
      put(g.t + 1, g.ro);
    } else {
      put(g.t, 0.0);
    }
  }
  return true;
}
// ... and what follows it on rho[0 .. T]: the monotone sequence, tau in lag order and its floor. ess = draws / tau.
__host__ __device__ __forceinline__ double ess_from_rho_of(double *rho, int T, int draws) {
  for (int t = 0; t <= T - 4;) {
    t += 2;
    const double prev = rho[t - 2] + rho[t - 1];
    if (rho[t] + rho[t + 1] > prev) rho[t] = rho[t + 1] = prev / 2.0;
  }
  double sum = 0.0;
  for (int t = 0; t < T; t++) sum += rho[t];
  double tau = -1.0 + 2.0 * sum + rho[T];
  const double floor_tau = ess_tau_floor(draws);
  if (tau < floor_tau) tau = floor_tau;
  return (double)draws / tau;
}
// one chain: its two halves of n draws
__host__ __device__ __forceinline__ double ess_from_rho(double *rho, int T, int n) { return ess_from_rho_of(rho, T, 2 * n); }

struct RowEssArgs {
  const double *scratch;  // [S][Tn] the tile's scores
  const double *y;        // of the tile's first row (kind 1)
  const double *aux;      // the per-sample constants: those of k_row_logdens (kind 1), cut[S][n_cut] (kind 0, mode 2)
  const double *table;    // [2S - 1] the rank-normalised values by twice the average rank
  double *out0, *out1, *out2, *out3;  // of the tile's first row
  int64_t Tn;
  int S, n_cut;
  int n_aux, aux_lds;     // the constants, in doubles, and whether they are staged in LDS behind the rows
  int P, R;               // S padded to a power of two, rows per workgroup
  int st, stv;            // doubles per row of v and z (S | 1) and of the sort buffer (P | 1): odd, the row-per-lane phases are conflict-free
  int M;                  // the chains the S samples are, chain after chain (S % M == 0, M <= ESS_MAX_CHAINS); last: the single-chain
                          // kernels, which do not read it, find every other argument where it was before chains were known
};

// LDS, in doubles: hdr[R][ESS_HDR], the values v[R][st], the work buffer z[R][st], the sort buffer sv[R][stv], the sample indices
// idx[R][P] (ints), the per-sample constants where they are staged
static size_t ess_lds_doubles(int R, int st, int stv, int P, size_t n_aux) {
  return (size_t)R * (ESS_HDR + 2 * (size_t)st + (size_t)stv + (size_t)(P + 1) / 2) + n_aux;
}

// E for the rows of a workgroup up to Geyer's truncation: a wavefront takes a row, four rows per round. Lanes 0 and 1 add up the
// halves' means; lane j then owns lag t0 + j of a batch of 64 and walks i in sample order (x_i at one LDS address for all lanes: a
// broadcast; x_{i+t} at consecutive addresses), for both halves. The batch's A(t) stay in the lanes' registers; Geyer's first
// loop, which every lane of the wavefront runs alike, reads them by shuffle and lane 0 stores the sequence in rho. The next
// batch is computed only if the loop has not truncated: the lags consumed are those of the definition. No barrier inside (the
// wavefronts make different numbers of batches). Leaves hdr[ESS_H_T] = T (-1: no diagnosis) and hdr[ESS_H_R] = sqrt(V / W).
// want_ess false: lag 0 alone, for R.
__device__ __forceinline__ void ess_rows_truncate(const double *x, int xs, double *rho, int rs, double *hdr, int R, int nr, int S,
                                                  bool want_ess) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int n = S / 2;
  for (int rb = 0; rb < R; rb += WG / WAVE) {
    const int r = rb + wave;
    if (r >= nr) continue;  // (one value for the wavefront)
    const double *xa = x + (size_t)r * xs, *xb = xa + (S - n);
    double *rr = rho + (size_t)r * rs, *h = hdr + r * ESS_HDR;
    const double x0_a = xa[0], x0_b = xb[0];
    double mu = 0.0;
    if (lane < 2) {
      const double *half = lane ? xb : xa;
      const double x0 = lane ? x0_b : x0_a;
      double sum = 0.0;
      for (int i = 0; i < n; i++) sum += half[i] - x0;
      mu = sum / (double)n;
    }
    const double mu_a = __shfl(mu, 0), mu_b = __shfl(mu, 1);  // (of the shifted halves)
    EssGeyer g{0, 1.0, 0.0};
    double W = 0.0, V = 0.0;
    bool done = false, ok = true;
    for (int t0 = 0; t0 < n && !done; t0 += WAVE) {
      const int t = t0 + lane;
      double A = 0.0;
      if (t < n && (want_ess || t == 0)) {
        const int m = n - t;
        double sa = 0.0, sb = 0.0;
        for (int i = 0; i < m; i++) {
          sa += ess_centered(xa[i], x0_a, mu_a) * ess_centered(xa[i + t], x0_a, mu_a);
          sb += ess_centered(xb[i], x0_b, mu_b) * ess_centered(xb[i + t], x0_b, mu_b);
        }
        A = ess_autocov(sa, sb, n);
      }
      if (t0 == 0) {
        const double A0 = __shfl(A, 0);
        W = ess_within(A0, n);
        V = ess_total(A0, x0_a + mu_a, x0_b + mu_b);
        ok = ess_within_ok(W);
        if (!ok || !want_ess) break;
        g.ro = ess_rho(W, __shfl(A, 1), V);
        if (lane == 0) {
          rr[0] = g.re;
          rr[1] = g.ro;
        }
      }
      done = ess_geyer_advance(
          g, n, t0 + WAVE < n ? t0 + WAVE : n, W, V, [&](int tt) { return __shfl(A, tt - t0); },
          [&](int tt, double value) {
            if (lane == 0) rr[tt] = value;
          });
    }
    if (lane == 0) {
      if (ok && want_ess && g.re > 0.0) rr[g.t] = g.re;
      h[ESS_H_T] = ok ? (double)g.t : -1.0;
      h[ESS_H_R] = ok ? sqrt(V / W) : __builtin_nan("");
    }
  }
}

// E for the rows of a workgroup up to Geyer's truncation, several chains: as ess_rows_truncate above with C = 2M sequences. Lanes
// 0 .. C - 1 add up the sequences' means, a sequence per lane; lane j then owns lag t0 + j of a batch of 64 and walks the chains in
// their order, and within a chain i in sample order for its two halves (x_i at one LDS address for all lanes: a broadcast; x_{i+t}
// at consecutive addresses). A sequence's first draw is read from the row and its mean comes by shuffle from the lane that added it
// up, outside the lanes' own loops: every lane of the wavefront takes part in a shuffle. At M = 1 every operation is the one
// ess_rows_truncate makes, in its order (the same bits); the single-chain form is kept beside this one because this text ran the
// single-chain calls 0.2 to 0.9 ms (up to 2.7 %) above the parent's range in four of six instantiations (Measured;
// profiles/diagnostics_chains_bench.txt).
__device__ __forceinline__ void ess_rows_truncate_chains(const double *x, int xs, double *rho, int rs, double *hdr, int R, int nr, int S,
                                                  int M, bool want_ess) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  const int L = S / M, n = L / 2, C = 2 * M;
  for (int rb = 0; rb < R; rb += WG / WAVE) {
    const int r = rb + wave;
    if (r >= nr) continue;  // (one value for the wavefront)
    const double *xr = x + (size_t)r * xs;
    double *rr = rho + (size_t)r * rs, *h = hdr + r * ESS_HDR;
    double mu = 0.0, mean = 0.0;  // of lane c's sequence: shifted by its first draw, and itself
    if (lane < C) {
      const double *seq = xr + ess_sequence_start(lane, L, n);
      const double x0 = seq[0];
      double sum = 0.0;
      for (int i = 0; i < n; i++) sum += seq[i] - x0;
      mu = sum / (double)n;
      mean = x0 + mu;
    }
    EssGeyer g{0, 1.0, 0.0};
    double W = 0.0, V = 0.0;
    bool done = false, ok = true;
    for (int t0 = 0; t0 < n && !done; t0 += WAVE) {
      const int t = t0 + lane;
      const int m = t < n && (want_ess || t == 0) ? n - t : 0;  // (a lane without a lag adds up nothing: A = 0)
      double acc = 0.0;
      for (int ch = 0; ch < M; ch++) {
        const double *xa = xr + ch * L, *xb = xa + (L - n);
        const double x0_a = xa[0], x0_b = xb[0];
        const double mu_a = __shfl(mu, 2 * ch), mu_b = __shfl(mu, 2 * ch + 1);
        double sa = 0.0, sb = 0.0;
        for (int i = 0; i < m; i++) {
          sa += ess_centered(xa[i], x0_a, mu_a) * ess_centered(xa[i + t], x0_a, mu_a);
          sb += ess_centered(xb[i], x0_b, mu_b) * ess_centered(xb[i + t], x0_b, mu_b);
        }
        acc = ess_autocov_add(acc, sa, sb, n);
      }
      const double A = ess_autocov_mean(acc, C);
      if (t0 == 0) {
        const double A0 = __shfl(A, 0);
        W = ess_within(A0, n);
        V = ess_total(A0, C, [&](int c) { return __shfl(mean, c); });
        ok = ess_within_ok(W);
        if (!ok || !want_ess) break;
        g.ro = ess_rho(W, __shfl(A, 1), V);
        if (lane == 0) {
          rr[0] = g.re;
          rr[1] = g.ro;
        }
      }
      done = ess_geyer_advance(
          g, n, t0 + WAVE < n ? t0 + WAVE : n, W, V, [&](int tt) { return __shfl(A, tt - t0); },
          [&](int tt, double value) {
            if (lane == 0) rr[tt] = value;
          });
    }
    if (lane == 0) {
      if (ok && want_ess && g.re > 0.0) rr[g.t] = g.re;
      h[ESS_H_T] = ok ? (double)g.t : -1.0;
      h[ESS_H_R] = ok ? sqrt(V / W) : __builtin_nan("");
    }
  }
}

// the bitonic network of k_row_psis over the (value, sample index) pairs of all R rows, P = S padded with +inf
__device__ __forceinline__ void ess_rows_sort(double *sv, int stv, int *idx, int P, int R) {
  const int tid = threadIdx.x, half = P >> 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int e = tid; e < R * half; e += WG) {
        const int r = e / half, c2 = e - r * half;
        const int i = ((c2 & ~(j - 1)) << 1) | (c2 & (j - 1));
        double *vr = sv + (size_t)r * stv;
        int *ir = idx + (size_t)r * P;
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
}

// Stage 2, one launch per row tile. KIND 0, the prediction value: SUB 0 the score, 1 Phi(score), 2 the expected class index
// under the sample's cutpoints. KIND 1, the likelihood: SUB the task of logdens_value. A workgroup brings R rows into LDS, every
// score turned into its value on the way (all threads); for the likelihood lane r then takes row r's maximum and all threads
// turn l into u = exp(l - max). Then
//   (b) E on v (ess_rows_truncate, rho in z), and a lane per row finishes it (ess_from_rho);
//   (c) v with the sample indices into the sort buffer, the bitonic network, and the thread at the first position of a tie group
//       walks the group and scatters its z by sample index (the thread at position 0 also keeps the two middle order statistics);
//       E on z, rho in the sort buffer, finished by a lane per row;
//   (d) |v - med| (ess_folded) into the sort buffer, sorted and ranked in the same way, and E's lag 0 on its z, for R alone;
//   (e) a lane per row takes the mean and the standard deviation (ddof = 1) of v in sample order and stores the four outputs.
// A chain of fewer than 8 draws (S / M < 8): NaN and nothing else.
// CHAINS: the samples are a.M chains (ess_rows_truncate_chains); else one chain, the text as it was before chains were known.
template <int KIND, int SUB, bool CHAINS>
__global__ __launch_bounds__(WG) void k_row_ess(RowEssArgs a) {
  extern __shared__ double ess_lds[];
  const int S = a.S, M = CHAINS ? a.M : 1, R = a.R, st = a.st, stv = a.stv, P = a.P, n_cut = a.n_cut;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int nr = (int)(a.Tn - r0 < R ? a.Tn - r0 : R);
  const int tid = threadIdx.x;
  const double nan = __builtin_nan("");
  if (S / M < 2 * ESS_MIN_HALF) {
    if (tid < nr) a.out0[r0 + tid] = a.out1[r0 + tid] = a.out2[r0 + tid] = a.out3[r0 + tid] = nan;
    return;
  }
  double *hdr = ess_lds, *v = hdr + (size_t)R * ESS_HDR, *z = v + (size_t)R * st, *sv = z + (size_t)R * st;
  int *idx = reinterpret_cast<int *>(sv + (size_t)R * stv);
  double *staged = sv + (size_t)R * stv + (size_t)R * ((P + 1) / 2);
  const int n = S / 2, draws = 2 * M * (S / M / 2);  // a half of one chain; the draws that the 2M sequences hold
  constexpr bool HAS_AUX = (KIND == 0 && SUB == 2) || (KIND == 1 && SUB != LOGDENS_CLASSIFICATION);
  const bool use_staged = HAS_AUX && a.aux_lds;
  if (use_staged) {
    for (int i = tid; i < a.n_aux; i += WG) staged[i] = a.aux[i];
    __syncthreads();
  }
  // (a) (called once with the LDS pointer and once with the global one, so that neither becomes a flat access)
  const auto fill = [&](const double *aux) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      double value = 0.0;
      if (r < nr) {
        const double score = a.scratch[(size_t)s * a.Tn + r0 + r];
        if constexpr (KIND == 0) {
          if constexpr (SUB == 0)
            value = score;
          else if constexpr (SUB == 1)
            value = (erf(score * 0.70710678118654752440) + 1.0) / 2.0;  // (the expression of k_score_store MODE 4 and k_dist_copy)
          else
            value = oprobit_expected(score, aux + (size_t)s * n_cut, n_cut);
        } else {
          const double yt = a.y[r0 + r];
          if constexpr (SUB == LOGDENS_REGRESSION)
            value = logdens_value<SUB>(yt, score, aux[s], aux[S + s], nullptr, 0);
          else if constexpr (SUB == LOGDENS_CLASSIFICATION)
            value = logdens_value<SUB>(yt, score, 0.0, 0.0, nullptr, 0);
          else
            value = logdens_value<SUB>(yt, score, 0.0, 0.0, aux + (size_t)s * n_cut, n_cut);
        }
      }
      v[r * st + s] = value;
    }
  };
  if (use_staged)
    fill(staged);
  else
    fill(a.aux);
  __syncthreads();
  if constexpr (KIND == 1) {
    if (tid < nr) {
      const double *row = v + tid * st;
      double mx = row[0];
      for (int s = 1; s < S; s++) mx = fmax(mx, row[s]);
      hdr[tid * ESS_HDR + ESS_H_MAX] = mx;  // (-inf: a density of 0 under every sample, the row's u are NaN)
    }
    __syncthreads();
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      if (r < nr) v[r * st + s] = exp(v[r * st + s] - hdr[r * ESS_HDR + ESS_H_MAX]);
    }
    __syncthreads();
  }
  // (b)
  if constexpr (CHAINS)
    ess_rows_truncate_chains(v, st, z, st, hdr, R, nr, S, M, true);
  else
    ess_rows_truncate(v, st, z, st, hdr, R, nr, S, true);
  __syncthreads();
  if (tid < nr) {
    double *h = hdr + tid * ESS_HDR;
    if (h[ESS_H_T] < 0.0)
      h[ESS_H_ESS_MEAN] = nan;
    else if constexpr (CHAINS)
      h[ESS_H_ESS_MEAN] = ess_from_rho_of(z + tid * st, (int)h[ESS_H_T], draws);
    else
      h[ESS_H_ESS_MEAN] = ess_from_rho(z + tid * st, (int)h[ESS_H_T], n);
  }
  __syncthreads();
  // (c) and (d)
  for (int pass = 0; pass < 2; pass++) {
    for (int i = tid; i < S * R; i += WG) {
      const int s = i / R, r = i - s * R;
      const double x = v[r * st + s];
      sv[r * stv + s] = pass == 0 ? x : ess_folded(x, hdr[r * ESS_HDR + ESS_H_MID_LO], hdr[r * ESS_HDR + ESS_H_MID_HI]);
      idx[r * P + s] = s;
    }
    for (int i = tid; i < (P - S) * R; i += WG) {
      const int s = S + i / R, r = i % R;
      sv[r * stv + s] = __builtin_inf();
      idx[r * P + s] = s;
    }
    __syncthreads();
    ess_rows_sort(sv, stv, idx, P, R);
    for (int e = tid; e < R * S; e += WG) {
      const int r = e / S, p = e - r * S;
      if (r >= nr) continue;
      const double *vr = sv + (size_t)r * stv;
      const int *ir = idx + (size_t)r * P;
      const double x = vr[p];
      if (p == 0 || vr[p - 1] != x) {
        int last = p;
        while (last + 1 < S && vr[last + 1] == x) last++;
        const double zv = a.table[ess_tie_table_index(p, last)];
        for (int q = p; q <= last; q++) {
          const int si = ir[q];  // (a padding index can stand here only if a value was NaN)
          if (si < S) z[r * st + si] = zv;
        }
      }
      if (p == 0 && pass == 0) {
        hdr[r * ESS_HDR + ESS_H_MID_LO] = vr[(S - 1) / 2];
        hdr[r * ESS_HDR + ESS_H_MID_HI] = vr[S / 2];
      }
    }
    __syncthreads();
    if constexpr (CHAINS)
      ess_rows_truncate_chains(z, st, sv, stv, hdr, R, nr, S, M, pass == 0);
    else
      ess_rows_truncate(z, st, sv, stv, hdr, R, nr, S, pass == 0);
    __syncthreads();
    if (pass == 0 && tid < nr) {
      double *h = hdr + tid * ESS_HDR;
      if (h[ESS_H_T] < 0.0)
        h[ESS_H_ESS_BULK] = nan;
      else if constexpr (CHAINS)
        h[ESS_H_ESS_BULK] = ess_from_rho_of(sv + tid * stv, (int)h[ESS_H_T], draws);
      else
        h[ESS_H_ESS_BULK] = ess_from_rho(sv + tid * stv, (int)h[ESS_H_T], n);
      h[ESS_H_R_BULK] = h[ESS_H_R];
    }
    __syncthreads();
  }
  // (e)
  if (tid < nr) {
    const double *row = v + tid * st, *h = hdr + tid * ESS_HDR;
    bool finite = true;
    double sum = 0.0, ss = 0.0;
    for (int s = 0; s < S; s++) {
      sum += row[s];
      finite = finite && fabs(row[s]) < __builtin_inf();
    }
    const double mean = sum / (double)S;
    for (int s = 0; s < S; s++) ss += (row[s] - mean) * (row[s] - mean);
    const double sd = sqrt(ss / (double)(S - 1)), ess = h[ESS_H_ESS_MEAN];
    a.out0[r0 + tid] = finite ? fmax(h[ESS_H_R_BULK], h[ESS_H_R]) : nan;
    a.out1[r0 + tid] = finite ? h[ESS_H_ESS_BULK] : nan;
    if constexpr (KIND == 0) {
      a.out2[r0 + tid] = finite ? ess : nan;
      a.out3[r0 + tid] = finite ? sd / sqrt(ess) : nan;
    } else {
      a.out2[r0 + tid] = finite ? ess / (double)S : nan;
      a.out3[r0 + tid] = finite ? sd / (mean * sqrt(ess)) : nan;
    }
  }
}

template <int KIND, int SUB, bool CHAINS>
static void launch_row_ess_form(hipStream_t s, const RowEssArgs &a, size_t lds) {
  static DeviceOnce raised;
  if (lds > 64 * 1024 && raised.need()) {  // above the default limit of dynamic LDS (opted into once per device)
    void (*const kernel)(RowEssArgs) = k_row_ess<KIND, SUB, CHAINS>;
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ESS_LDS_MAX_BYTES));
    raised.mark();
  }
  hipLaunchKernelGGL((k_row_ess<KIND, SUB, CHAINS>), dim3((unsigned)cdiv(a.Tn, a.R)), dim3(WG), lds, s, a);
}
// Sized next to launch_row_psis' arithmetic: R rows of 9 + 2 (S | 1) + (P | 1) + P / 2 doubles within ESS_LDS_BYTES, at most
// ESS_MAX_ROWS and never less than one row (S = 95: 392 doubles, R = 20; S = 1024: 3 596, R = 2; S = 4096: 14 348 doubles =
// 114 784 B, R = 1); the constants behind them where the budget still holds them.
static void launch_row_ess(hipStream_t s, int kind, int sub, RowEssArgs &a) {
  int P = 1;
  while (P < a.S) P <<= 1;
  a.P = P;
  a.st = a.S | 1;
  a.stv = P | 1;
  const size_t row = ess_lds_doubles(1, a.st, a.stv, P, 0);
  const size_t budget = ESS_LDS_BYTES / sizeof(double);
  a.R = (int)std::min<int64_t>(std::max<int64_t>(1, std::min<int64_t>(ESS_MAX_ROWS, (int64_t)(budget / row))), a.Tn);
  const size_t rows = ess_lds_doubles(a.R, a.st, a.stv, P, 0);
  a.aux_lds = a.n_aux > 0 && rows + (size_t)a.n_aux <= budget;
  const size_t lds = (rows + (a.aux_lds ? (size_t)a.n_aux : 0)) * sizeof(double);
  logdens_with_task(sub, [&](auto sub_c) {
    constexpr int SUB = decltype(sub_c)::value;
    if (kind == 0)
      a.M > 1 ? launch_row_ess_form<0, SUB, true>(s, a, lds) : launch_row_ess_form<0, SUB, false>(s, a, lds);
    else
      a.M > 1 ? launch_row_ess_form<1, SUB, true>(s, a, lds) : launch_row_ess_form<1, SUB, false>(s, a, lds);
  });
}

// table[j] = Phi^-1((1 + j / 2 - 3 / 8) / (S + 1 / 4)), j = 0 .. 2S - 2: the rank-normalised value of the average rank 1 + j / 2
static void ess_rank_z_table(int S, double *out) {
  for (int j = 0; j < 2 * S - 1; j++) out[j] = mfm_std_normal_quantile((1.0 + (double)j / 2.0 - 0.375) / ((double)S + 0.25));
}

// E of one sequence of M chains on the host, sequentially, through the scalar pieces and in the summation orders of k_row_ess
static void ess_row_host(int S, int M, const double *x, double *out_ess, double *out_rhat) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  *out_ess = *out_rhat = nan;
  const int L = S / M, n = L / 2, C = 2 * M;
  if (n < ESS_MIN_HALF) return;
  std::vector<double> mu((size_t)C), mean((size_t)C);  // of the shifted sequences, and of the sequences
  for (int c = 0; c < C; c++) {
    const double *seq = x + ess_sequence_start(c, L, n);
    double sum = 0.0;
    for (int i = 0; i < n; i++) sum += seq[i] - seq[0];
    mu[(size_t)c] = sum / (double)n;
    mean[(size_t)c] = seq[0] + mu[(size_t)c];
  }
  const auto A = [&](int t) {
    double acc = 0.0;
    for (int ch = 0; ch < M; ch++) {
      const double *xa = x + ch * L, *xb = xa + (L - n);
      const double x0_a = xa[0], x0_b = xb[0], mu_a = mu[(size_t)(2 * ch)], mu_b = mu[(size_t)(2 * ch + 1)];
      double sa = 0.0, sb = 0.0;
      for (int i = 0; i < n - t; i++) {
        sa += ess_centered(xa[i], x0_a, mu_a) * ess_centered(xa[i + t], x0_a, mu_a);
        sb += ess_centered(xb[i], x0_b, mu_b) * ess_centered(xb[i + t], x0_b, mu_b);
      }
      acc = ess_autocov_add(acc, sa, sb, n);
    }
    return ess_autocov_mean(acc, C);
  };
  const double A0 = A(0), W = ess_within(A0, n), V = ess_total(A0, C, [&](int c) { return mean[(size_t)c]; });
  if (!ess_within_ok(W)) return;
  std::vector<double> rho((size_t)n + 2, 0.0);
  EssGeyer g{0, 1.0, ess_rho(W, A(1), V)};
  rho[0] = g.re;
  rho[1] = g.ro;
  ess_geyer_advance(g, n, n, W, V, A, [&](int t, double value) { rho[(size_t)t] = value; });
  if (g.re > 0.0) rho[(size_t)g.t] = g.re;
  *out_ess = ess_from_rho_of(rho.data(), g.t, C * n);
  *out_rhat = std::sqrt(V / W);
}

// The checks of a diagnostics call; nothing here touches the device. The call is a LogdensCall whose task is the likelihood's task
// (kind 1) or the value's mode (kind 0), and whose out_lpd / out_mean / out_var are the first three outputs.
static void ess_check_chains(int32_t n_chains, int count) {
  if (n_chains < 1) throw Error(MFM_ERR_INVALID, "n_chains must be at least 1, got " + std::to_string(n_chains));
  if (n_chains > ESS_MAX_CHAINS)
    throw Error(MFM_ERR_INVALID, "chain diagnostics combine at most " + std::to_string(ESS_MAX_CHAINS) + " chains, got " + std::to_string(n_chains));
  if (count % n_chains != 0)
    throw Error(MFM_ERR_INVALID, "the chains must be of equal length: " + std::to_string(count) + " samples are not a multiple of n_chains = " +
                                     std::to_string(n_chains));
}
static void ess_check(int32_t kind, const LogdensCall &c, const double *out3, int64_t N, int count, int32_t n_chains) {
  ess_check_chains(n_chains, count);
  if (kind < 0 || kind > 1) throw Error(MFM_ERR_INVALID, "bad kind (0: the prediction value, 1: the likelihood)");
  if (kind == 1) {
    logdens_check(c, N, count);
  } else {
    if (c.task < 0 || c.task > 2) throw Error(MFM_ERR_INVALID, "bad mode (0: score, 1: Phi(score), 2: the expected class index of ordered probit)");
    check_tiling(c.tile_rows, c.chunk_samples);
    if (c.precisions) throw Error(MFM_ERR_INVALID, "noise precisions do not apply to the prediction value (kind 0)");
    if (c.task == 2) {
      if (c.n_cut < 1) throw Error(MFM_ERR_INVALID, "the expected class index needs at least one cutpoint per sample");
      if (!c.cutpoints) throw Error(MFM_ERR_INVALID, "the expected class index needs the samples' cutpoints");
      check_cutpoints(c.cutpoints, count, c.n_cut);
    } else if (c.cutpoints || c.n_cut != 0) {
      throw Error(MFM_ERR_INVALID, "cutpoints apply to the expected class index (mode 2) only");
    }
    if (N > 0 && (!c.out_lpd || !c.out_mean || !c.out_var)) throw Error(MFM_ERR_INVALID, "chain diagnostics need their four output arrays");
  }
  if (N > 0 && !out3) throw Error(MFM_ERR_INVALID, "chain diagnostics need their four output arrays");
  if (count > DIST_MAX_S)
    throw Error(MFM_ERR_INVALID, "chain diagnostics are computed over at most " + std::to_string(DIST_MAX_S) + " samples, got " + std::to_string(count));
}

static void design_ess(mfm_design *d, const SampleView &v, int32_t kind, const LogdensCall &c, double *out3, int32_t n_chains) {
  const int count = v.count();
  check_sample_source(d, v);
  hipStream_t s = d->stream;
  const size_t N = (size_t)d->N;
  if (N == 0) return;
  const size_t n_table = 2 * (size_t)count - 1;
  const int64_t T = dist_tiles_reserve(d, v, c.tile_rows, N * 4 + n_table);  // the four outputs, and the table behind them
  LogdensConstants k{nullptr, 0};
  if (kind == 1) {
    k = logdens_upload(d, s, c, d->N, count);
  } else if (c.task == 2) {
    const size_t n = (size_t)count * c.n_cut;
    if (d->cut.n < n) d->cut.alloc(n);
    MFM_HIP_CHECK(hipMemcpyAsync(d->cut.p, c.cutpoints, n * sizeof(double), hipMemcpyHostToDevice, s));
    k = {d->cut.p, n};
  }
  std::vector<double> table(n_table);  // (it lives until dist_tiles_run has waited for the stream)
  ess_rank_z_table(count, table.data());
  MFM_HIP_CHECK(hipMemcpyAsync(d->dist_out.p + 4 * N, table.data(), n_table * sizeof(double), hipMemcpyHostToDevice, s));
  RowEssArgs a;
  std::memset(&a, 0, sizeof(a));
  a.scratch = d->dist_scratch.p;
  a.aux = k.aux;
  a.n_aux = (int)k.n_aux;
  a.table = d->dist_out.p + 4 * N;
  a.S = count;
  a.M = n_chains;
  a.n_cut = c.task == 2 ? c.n_cut : 0;
  const auto stage2 = [&](int64_t r0, int64_t Tn) {
    a.Tn = Tn;
    a.y = kind == 1 ? d->dist_y.p + r0 : nullptr;
    a.out0 = d->dist_out.p + r0;
    a.out1 = d->dist_out.p + N + r0;
    a.out2 = d->dist_out.p + 2 * N + r0;
    a.out3 = d->dist_out.p + 3 * N + r0;
    launch_row_ess(s, kind, c.task, a);
  };
  dist_tiles_run(d, v, T, 0, c.chunk_samples, nullptr, {{c.out_lpd, 0, N}, {c.out_mean, N, N}, {c.out_var, 2 * N, N}, {out3, 3 * N, N}}, stage2);
}

}  // namespace mfm

extern "C" {

int mfm_design_ess_chains_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t n_chains, int32_t kind, int32_t mode_or_task,
                                const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                                int32_t chunk_samples, double *out0, double *out1, double *out2, double *out3) {
  MFM_TRY(d)
  const LogdensCall c{mode_or_task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out0, out1, out2, nullptr, nullptr};
  ess_check(kind, c, out3, d->N, std::max(count, 0), n_chains);
  design_ess(d, samples_of_store(st, first, count), kind, c, out3, n_chains);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_ess_chains(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t n_chains,
                          int32_t kind, int32_t mode_or_task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                          int64_t tile_rows, int32_t chunk_samples, double *out0, double *out1, double *out2, double *out3) {
  MFM_TRY(d)
  const LogdensCall c{mode_or_task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out0, out1, out2, nullptr, nullptr};
  ess_check(kind, c, out3, d->N, std::max(n_samples, 0), n_chains);
  store_check_fraction(d->D, rank, n_samples);
  design_ess(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), kind, c, out3, n_chains);
  MFM_CATCH(d)
}

// one chain
int mfm_design_ess_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t kind, int32_t mode_or_task, const double *y,
                         const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples,
                         double *out0, double *out1, double *out2, double *out3) {
  return mfm_design_ess_chains_store(d, st, first, count, 1, kind, mode_or_task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples, out0,
                                     out1, out2, out3);
}
int mfm_design_ess(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t kind,
                   int32_t mode_or_task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                   int32_t chunk_samples, double *out0, double *out1, double *out2, double *out3) {
  return mfm_design_ess_chains(d, rank, n_samples, w0s, ws, Vs, 1, kind, mode_or_task, y, precisions, n_cut, cutpoints, tile_rows, chunk_samples,
                               out0, out1, out2, out3);
}

// E of one sequence of n_chains chains on the host, by the scalar pieces the kernel runs (no device): x[S], chain after chain; chains
// of fewer than 8 draws give NaN
int mfm_ess_row_chains(int32_t S, int32_t n_chains, const double *x, double *out_ess, double *out_rhat) {
  if (S < 1 || S > mfm::DIST_MAX_S || !x || !out_ess || !out_rhat) {
    g_global_error = "a sequence of 1 to " + std::to_string(mfm::DIST_MAX_S) + " draws and the two outputs are needed";
    return MFM_ERR_INVALID;
  }
  try {
    mfm::ess_check_chains(n_chains, S);
    mfm::ess_row_host(S, n_chains, x, out_ess, out_rhat);
  } catch (const mfm::Error &e) {
    g_global_error = e.what();
    return e.code;
  } catch (const std::bad_alloc &) {
    g_global_error = "host out of memory";
    return MFM_ERR_RUNTIME;
  }
  return MFM_OK;
}
int mfm_ess_row(int32_t S, const double *x, double *out_ess, double *out_rhat) { return mfm_ess_row_chains(S, 1, x, out_ess, out_rhat); }

// what ess_check refuses of a chain count over n_samples samples, for a caller that has to know before it makes a design
int mfm_ess_check_chains(int32_t n_samples, int32_t n_chains) {
  try {
    mfm::ess_check_chains(n_chains, std::max(n_samples, 0));
  } catch (const mfm::Error &e) {
    g_global_error = e.what();
    return e.code;
  }
  return MFM_OK;
}
int32_t mfm_ess_max_chains(void) { return mfm::ESS_MAX_CHAINS; }

// the rank-normalised values of S draws by twice the average rank: out[2S - 1]
int mfm_rank_z_table(int32_t S, double *out) {
  if (S < 1 || S > mfm::DIST_MAX_S || !out) {
    g_global_error = "1 to " + std::to_string(mfm::DIST_MAX_S) + " draws and the output are needed";
    return MFM_ERR_INVALID;
  }
  mfm::ess_rank_z_table(S, out);
  return MFM_OK;
}

}  // extern "C"
