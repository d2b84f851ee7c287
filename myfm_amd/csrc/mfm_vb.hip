// mfm_vb.hip -- the variational FM trainer (VariationalFMTrainer, include/myfm/variational.hpp) on the device: the O(N),
// O(nnz) and O(D K) steps of one iteration behind the mfm_vb_* entry points of include/myfm_hip.h. The host layer
// (csrc/_myfm.cpp, create_train_vfm) runs the O(G K) hyper-parameter arithmetic between the calls, in the reference's order.
//
// Layout: the main table as CSR (score pass, per-factor cache build) and as CSC walked level by level (the coordinate sweeps):
// columns of one level share no row, so their updates commute and one launch runs them side by side, one wavefront per column;
// the levels run in order, so every column sees the updates of all columns before it (column_levels, mfm_common.hpp).
// Per row: e, and for the factor being swept q, x2s, x3sv. Every sum has a fixed association (lane-strided, then a butterfly
// over the wavefront or a tree over the workgroup, then one workgroup over the partials), so a rerun is bit-identical; no
// floating-point atomics.
//
// Row-sharded (a communicator set: mfm_vb_set_allreduce / mfm_vb_comm_init): this context holds a contiguous slice of the rows
// and a replica of the model. A column's sums must cross the ranks before its update, so every level runs as
//   k_vb_stats_w / k_vb_stats_v -> S (2 | 4 doubles per column of the level) -> ONE all-reduce of S -> k_vb_apply_w / k_vb_apply_v
// with S holding only terms that are additive over rows; everything that multiplies by v_old, alpha or lambda happens in the
// apply kernel, from the reduced sums, which are the same on every rank: every rank writes the model entry itself and the
// replicas stay bit-identical without a broadcast. The four score sums are all-reduced as one buffer per mfm_vb_update_e.
// Per iteration: (K + 1) * (non-empty levels) + 1 collectives.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mfm_comm.hpp"
#include "mfm_common.hpp"
#include "mfm_vb.hpp"

namespace mfm {
namespace vb {

constexpr int WG = 256;
constexpr int WAVE = 64;
constexpr int COLS_PER_WG = WG / WAVE;
constexpr int MAX_PARTS = 4096;  // workgroups of the score pass (rows beyond are walked grid-strided)

// butterfly over the 64 lanes: every lane ends with the same value, grouped the same way on every run
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
  return v;
}

// tree over the workgroup; the result in thread 0
template <int M>
__device__ __forceinline__ void wg_sum(double (&v)[M], double (*lds)[WG]) {
#pragma unroll
  for (int m = 0; m < M; m++) lds[m][threadIdx.x] = v[m];
  __syncthreads();
  for (int s = WG / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int m = 0; m < M; m++) lds[m][threadIdx.x] += lds[m][threadIdx.x + s];
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < M; m++) v[m] = lds[m][0];
}

// update_e_and_var (variational.hpp:715-833) and the task's residual (:835-867). mode 0: e -= y (initialize_e :234-241 for
// both tasks, update_e for regression); mode 1: classification, e -= E[z] of the truncated normal and the likelihood term
// lnZ + (E[z] - pred)^2 / 2. Per-workgroup partials of (sum e, sum e^2, sum of the per-row variance terms, likelihood term).
__global__ __launch_bounds__(WG) void k_vb_score(int64_t N, int64_t D, int K, const int64_t *__restrict__ ptr,
                                                 const int32_t *__restrict__ idx, const double *__restrict__ val, double w0,
                                                 const double *__restrict__ w, const double *__restrict__ wv,
                                                 const double *__restrict__ V, const double *__restrict__ Vv,
                                                 const double *__restrict__ y, int mode, double *__restrict__ e,
                                                 double *__restrict__ part) {
  __shared__ double lds[4][WG];
  double acc[4] = {0, 0, 0, 0};
  for (int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x; t < N; t += (int64_t)gridDim.x * WG) {
    const int64_t b = ptr[t], en = ptr[t + 1];
    double et = w0, vt = 0;
    for (int64_t p = b; p < en; p++) {
      const double x = val[p];
      const int32_t j = idx[p];
      et += x * w[j];
      vt += x * x * wv[j];
    }
    for (int f = 0; f < K; f++) {
      const double *Vf = V + (int64_t)f * D, *Vvf = Vv + (int64_t)f * D;
      double q = 0, q_s = 0, x2s = 0, x3sv = 0, x4s2 = 0, x4sv2 = 0;
      for (int64_t p = b; p < en; p++) {
        const double x = val[p], x2 = x * x, x4 = x2 * x2;
        const int32_t j = idx[p];
        const double v = Vf[j], s = Vvf[j];
        q += x * v;
        q_s += x2 * v * v;
        x2s += x2 * s;
        x3sv += x2 * x * s * v;
        x4s2 += x4 * s * s;
        x4sv2 += x4 * s * v * v;
      }
      et += 0.5 * (q * q - q_s);
      vt += (q * q * x2s + 0.5 * x2s * x2s - 2 * x3sv * q - 0.5 * x4s2 + x4sv2);
    }
    double lik = 0;
    if (mode == 0) {
      et -= y[t];
    } else {
      const double pred = et;
      const VbMoments n = y[t] > 0 ? vb_truncnorm_left(pred) : vb_truncnorm_right(pred);
      et -= n.mean;
      lik = n.lnz + (n.mean - pred) * (n.mean - pred) / 2;
    }
    e[t] = et;
    acc[0] += et;
    acc[1] += et * et;
    acc[2] += vt;
    acc[3] += lik;
  }
  wg_sum<4>(acc, lds);
  if (threadIdx.x == 0)
    for (int m = 0; m < 4; m++) part[(int64_t)blockIdx.x * 4 + m] = acc[m];
}

// the partials of k_vb_score in one workgroup: out[m] = sum over parts of part[4 p + m]
__global__ __launch_bounds__(WG) void k_vb_reduce(const double *__restrict__ part, int n, double *__restrict__ out) {
  __shared__ double lds[4][WG];
  double acc[4] = {0, 0, 0, 0};
  for (int p = threadIdx.x; p < n; p += WG)
    for (int m = 0; m < 4; m++) acc[m] += part[(int64_t)p * 4 + m];
  wg_sum<4>(acc, lds);
  if (threadIdx.x == 0)
    for (int m = 0; m < 4; m++) out[m] = acc[m];
}

__global__ void k_vb_shift(int64_t N, double *__restrict__ e, double delta) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t < N) e[t] += delta;
}

// update_w (variational.hpp:363-393) for the columns of one level: one wavefront per column
__global__ __launch_bounds__(WG) void k_vb_sweep_w(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const int32_t *__restrict__ gidx, double alpha,
                                                   const double *__restrict__ lam, const double *__restrict__ mu,
                                                   double *__restrict__ w, double *__restrict__ wv, double *__restrict__ e) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;  // (whole wavefronts)
  const int32_t j = cols[c];
  const int32_t g = gidx[j];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double w_old = w[j];
  double s2 = 0, s1 = 0;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    s2 += x * x;
    s1 += x * (e[ridx[p]] - x * w_old);
  }
  s2 = wave_sum(s2);
  s1 = wave_sum(s1);
  const double square = lam[g] + alpha * s2;
  const double linear = -alpha * s1 + lam[g] * mu[g];
  const double w_new = linear / square;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    e[r] = (e[r] - x * w_old) + x * w_new;
  }
  if (lane == 0) {
    w[j] = w_new;
    wv[j] = 1 / square;
  }
}

// row-sharded update_w, first half: per column of the level (sum x^2, sum x (e - x w_old)) over the LOCAL rows -> S[2 c ..]
__global__ __launch_bounds__(WG) void k_vb_stats_w(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const double *__restrict__ w, const double *__restrict__ e,
                                                   double *__restrict__ S) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;  // (whole wavefronts)
  const int32_t j = cols[c];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double w_old = w[j];
  double s2 = 0, s1 = 0;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    s2 += x * x;
    s1 += x * (e[ridx[p]] - x * w_old);
  }
  s2 = wave_sum(s2);
  s1 = wave_sum(s1);
  if (lane == 0) {
    S[(int64_t)c * 2] = s2;
    S[(int64_t)c * 2 + 1] = s1;
  }
}

// second half: w_new and 1 / square from the sums over ALL ranks' rows (k_vb_sweep_w's expressions), e of the local rows
__global__ __launch_bounds__(WG) void k_vb_apply_w(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const int32_t *__restrict__ gidx, double alpha,
                                                   const double *__restrict__ lam, const double *__restrict__ mu,
                                                   const double *__restrict__ S, double *__restrict__ w,
                                                   double *__restrict__ wv, double *__restrict__ e) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;
  const int32_t j = cols[c];
  const int32_t g = gidx[j];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double w_old = w[j];
  const double s2 = S[(int64_t)c * 2], s1 = S[(int64_t)c * 2 + 1];
  const double square = lam[g] + alpha * s2;
  const double linear = -alpha * s1 + lam[g] * mu[g];
  const double w_new = linear / square;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    e[r] = (e[r] - x * w_old) + x * w_new;
  }
  if (lane == 0) {
    w[j] = w_new;
    wv[j] = 1 / square;
  }
}

// the per-row cache of one factor (variational.hpp:452-465): q, x2s, x3sv
__global__ void k_vb_cache(int64_t N, const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                           const double *__restrict__ val, const double *__restrict__ Vf, const double *__restrict__ Vvf,
                           double *__restrict__ q, double *__restrict__ x2s, double *__restrict__ x3sv) {
  const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (t >= N) return;
  double a = 0, b2 = 0, b3 = 0;
  for (int64_t p = ptr[t]; p < ptr[t + 1]; p++) {
    const double x = val[p];
    const int32_t j = idx[p];
    a += x * Vf[j];
    b2 += x * x * Vvf[j];
    b3 += x * x * x * Vvf[j] * Vf[j];
  }
  q[t] = a;
  x2s[t] = b2;
  x3sv[t] = b3;
}

// update_V, main table (variational.hpp:505-554) for the columns of one level and one factor: one wavefront per column
__global__ __launch_bounds__(WG) void k_vb_sweep_v(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const int32_t *__restrict__ gidx, double alpha,
                                                   const double *__restrict__ lam, const double *__restrict__ mu,
                                                   double *__restrict__ Vf, double *__restrict__ Vvf, double *__restrict__ e,
                                                   double *__restrict__ q, double *__restrict__ x2s, double *__restrict__ x3sv) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;
  const int32_t j = cols[c];
  const int32_t g = gidx[j];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double v_old = Vf[j], s_old = Vvf[j];
  double sq = 0, lin = 0, sq_var = 0, lin_var = 0;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    const double h = x * (q[r] - x * v_old);
    double a2 = x2s[r], a3 = x3sv[r];
    a2 -= x * x * s_old;
    a3 -= x * x * x * s_old * v_old;
    sq += h * h;
    lin += (-e[r]) * h;
    sq_var += a2 * x * x;
    lin_var += h * a2 - x * a3;
  }
  sq = wave_sum(sq);
  lin = wave_sum(lin);
  sq_var = wave_sum(sq_var);
  lin_var = wave_sum(lin_var);
  lin += sq * v_old;
  lin -= lin_var;
  sq += sq_var;
  sq *= alpha;
  lin *= alpha;
  sq += lam[g];
  lin += lam[g] * mu[g];
  const double v_new = lin / sq, s_new = 1 / sq;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    const double h = x * (q[r] - x * v_old);
    q[r] += x * (v_new - v_old);
    e[r] += h * (v_new - v_old);
    x2s[r] += x * x * (s_new - s_old);
    x3sv[r] += x * x * x * (s_new * v_new - s_old * v_old);
  }
  if (lane == 0) {
    Vf[j] = v_new;
    Vvf[j] = s_new;
  }
}

// row-sharded update_V, first half: (sq, lin, sq_var, lin_var) of k_vb_sweep_v over the LOCAL rows, as they stand before
// `lin += sq * v_old` -> S[4 c ..]
__global__ __launch_bounds__(WG) void k_vb_stats_v(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const double *__restrict__ Vf, const double *__restrict__ Vvf,
                                                   const double *__restrict__ e, const double *__restrict__ q,
                                                   const double *__restrict__ x2s, const double *__restrict__ x3sv,
                                                   double *__restrict__ S) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;
  const int32_t j = cols[c];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double v_old = Vf[j], s_old = Vvf[j];
  double sq = 0, lin = 0, sq_var = 0, lin_var = 0;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    const double h = x * (q[r] - x * v_old);
    double a2 = x2s[r], a3 = x3sv[r];
    a2 -= x * x * s_old;
    a3 -= x * x * x * s_old * v_old;
    sq += h * h;
    lin += (-e[r]) * h;
    sq_var += a2 * x * x;
    lin_var += h * a2 - x * a3;
  }
  sq = wave_sum(sq);
  lin = wave_sum(lin);
  sq_var = wave_sum(sq_var);
  lin_var = wave_sum(lin_var);
  if (lane == 0) {
    double *o = S + (int64_t)c * 4;
    o[0] = sq;
    o[1] = lin;
    o[2] = sq_var;
    o[3] = lin_var;
  }
}

// second half: v_new and s_new from the sums over ALL ranks' rows (k_vb_sweep_v's expressions), the state of the local rows
__global__ __launch_bounds__(WG) void k_vb_apply_v(const int32_t *__restrict__ cols, int n, const int64_t *__restrict__ cptr,
                                                   const int32_t *__restrict__ ridx, const double *__restrict__ cval,
                                                   const int32_t *__restrict__ gidx, double alpha,
                                                   const double *__restrict__ lam, const double *__restrict__ mu,
                                                   const double *__restrict__ S, double *__restrict__ Vf,
                                                   double *__restrict__ Vvf, double *__restrict__ e, double *__restrict__ q,
                                                   double *__restrict__ x2s, double *__restrict__ x3sv) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = blockIdx.x * COLS_PER_WG + (threadIdx.x / WAVE);
  if (c >= n) return;
  const int32_t j = cols[c];
  const int32_t g = gidx[j];
  const int64_t b = cptr[j], en = cptr[j + 1];
  const double v_old = Vf[j], s_old = Vvf[j];
  const double *in = S + (int64_t)c * 4;
  double sq = in[0], lin = in[1];
  const double sq_var = in[2], lin_var = in[3];
  lin += sq * v_old;
  lin -= lin_var;
  sq += sq_var;
  sq *= alpha;
  lin *= alpha;
  sq += lam[g];
  lin += lam[g] * mu[g];
  const double v_new = lin / sq, s_new = 1 / sq;
  for (int64_t p = b + lane; p < en; p += WAVE) {
    const double x = cval[p];
    const int32_t r = ridx[p];
    const double h = x * (q[r] - x * v_old);
    q[r] += x * (v_new - v_old);
    e[r] += h * (v_new - v_old);
    x2s[r] += x * x * (s_new - s_old);
    x3sv[r] += x * x * x * (s_new * v_new - s_old * v_old);
  }
  if (lane == 0) {
    Vf[j] = v_new;
    Vvf[j] = s_new;
  }
}

// per (slot, group): slot 0 = (w, w_var), slot 1 + f = (V[:, f], V_var[:, f]); one workgroup each over the group's features:
// sum theta, sum ((theta - mu)^2 + mu_var + var), sum log var (update_lambda_generic :269-295, update_mu_generic :298-318, the
// weight terms of the ELBO :880-917)
__global__ __launch_bounds__(WG) void k_vb_group_stats(int64_t D, int G, int s0, const int32_t *__restrict__ gfeat,
                                                       const int64_t *__restrict__ gptr, const double *__restrict__ w,
                                                       const double *__restrict__ wv, const double *__restrict__ V,
                                                       const double *__restrict__ Vv, const double *__restrict__ mu,
                                                       const double *__restrict__ mu_var, double *__restrict__ out) {
  __shared__ double lds[3][WG];
  const int s = s0 + (int)blockIdx.x / G, g = (int)blockIdx.x % G;
  const double *th = s == 0 ? w : V + (int64_t)(s - 1) * D;
  const double *va = s == 0 ? wv : Vv + (int64_t)(s - 1) * D;
  const double m = mu[(int64_t)s * G + g], mv = mu_var[(int64_t)s * G + g];
  double acc[3] = {0, 0, 0};
  for (int64_t p = gptr[g] + threadIdx.x; p < gptr[g + 1]; p += WG) {
    const int32_t j = gfeat[p];
    const double dev = th[j] - m;
    acc[0] += th[j];
    acc[1] += dev * dev + mv + va[j];
    acc[2] += log(va[j]);
  }
  wg_sum<3>(acc, lds);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; k++) out[(int64_t)blockIdx.x * 3 + k] = acc[k];
}

}  // namespace vb
}  // namespace mfm

using namespace mfm;

struct mfm_vb {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  std::string err;
  Comm comm;  // row-sharded mode: set before mfm_vb_finalize
  int64_t N_total = 0, row_offset = 0;  // (mfm_vb_set_shard; unsharded: N_total == N)
  std::vector<int32_t> given_levels;    // mfm_vb_set_levels: the schedule of the GLOBAL expanded design
  int64_t N = 0, D = 0;
  int K = 0, G = 0;
  double w0 = 0, w0_var = 0;
  int32_t n_levels = 0;
  std::vector<int64_t> level_ptr;  // columns of level l: order[level_ptr[l], level_ptr[l + 1])
  std::vector<int32_t> level_order;
  DevBuf<int64_t> ptr, cptr, gptr;
  DevBuf<int32_t> idx, ridx, order, gidx, gfeat;
  DevBuf<double> val, cval, y, w, wv, V, Vv, e, q, x2s, x3sv, part, red, hyp, stats;
  DevBuf<double> S;  // row-sharded: the sums of one level's columns (4 doubles per column of the largest level)
  int n_parts = 0;
  // staged by mfm_vb_create / mfm_vb_add_block until mfm_vb_finalize
  struct Block {
    HostCsr X;
    std::vector<int64_t> map;
  };
  HostCsr main;
  std::vector<Block> blocks;
  std::vector<double> y_host;
  bool finalized = false;

  ~mfm_vb() {
    if (comm.nccl) {  // (before the stream it is enqueued on goes)
      (void)Rccl::get().CommDestroy(comm.nccl);
      comm.nccl = nullptr;
    }
    if (stream && own_stream) (void)hipStreamDestroy(stream);
  }
  bool sharded() const { return comm.active(); }
  void use() { MFM_HIP_CHECK(hipSetDevice(device)); }
  void put_hyp(const double *a, size_t na, const double *b, size_t nb) {  // small per-call uploads: [a | b]
    std::vector<double> h(a, a + na);
    h.insert(h.end(), b, b + nb);
    if (h.empty()) return;
    if (hyp.n < h.size()) throw Error(MFM_ERR_INVALID, "hyper-parameter upload larger than its buffer");
    MFM_HIP_CHECK(hipMemcpyAsync(hyp.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    MFM_HIP_CHECK(hipStreamSynchronize(stream));  // (h is freed on return)
  }
  template <class F>
  void each_level(F f) {
    for (int32_t l = 0; l < n_levels; l++) {
      const int n = (int)(level_ptr[l + 1] - level_ptr[l]);
      if (n) f(order.p + level_ptr[l], n, cdiv_(n, vb::COLS_PER_WG));
    }
  }
  static int cdiv_(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
};

namespace {
template <class F>
int vb_guard(mfm_vb *v, F f, bool need_finalized = true) {
  if (!v) return MFM_ERR_INVALID;
  try {
    v->use();
    if (need_finalized && !v->finalized) throw Error(MFM_ERR_INVALID, "call mfm_vb_finalize first");
    f();
    return MFM_OK;
  } catch (const Error &ex) {
    v->err = ex.what();
    return ex.code;
  } catch (const std::exception &ex) {
    v->err = ex.what();
    return MFM_ERR_RUNTIME;
  }
}
thread_local std::string g_vb_error;

// The design the sweeps walk: the main table with every relation block's row appended to the train rows that map to
// it, block columns after the main table's (the feature order of BaseFMTrainer.hpp:58-105). The reference's block
// caches (variational.hpp:388-447, :557-710, :728-827) are sums over the train rows of a block row, so this is the same
// iteration in exact arithmetic; tests/vb_ref.py restates the block algebra and holds the two to rounding.
// X: the expanded table, Xt: its CSC. Shared by mfm_vb_finalize and mfm_vb_design_levels.
void vb_expand_design(const HostCsr &main, const std::vector<mfm_vb::Block> &blocks, HostCsr &X, HostCsr &Xt) {
  const int64_t N = main.rows;
  int64_t D = main.cols;
  std::vector<int64_t> offset;
  for (auto &b : blocks) {
    offset.push_back(D);
    D += b.X.cols;
  }
  X.rows = N;
  X.cols = D;
  X.ptr.assign((size_t)N + 1, 0);
  for (int64_t t = 0; t < N; t++) {
    int64_t n = main.ptr[t + 1] - main.ptr[t];
    for (auto &b : blocks) n += b.X.ptr[b.map[t] + 1] - b.X.ptr[b.map[t]];
    X.ptr[t + 1] = X.ptr[t] + n;
  }
  if (X.ptr[N] >= (int64_t)2147483647) throw Error(MFM_ERR_INVALID, "nnz must be < 2^31 (relation blocks expanded)");
  X.idx.resize((size_t)X.ptr[N]);
  X.val.resize((size_t)X.ptr[N]);
  // a column twice in one row would put the row twice into one CSC column, and two lanes of a sweep would update that
  // row's state at the same time
  std::vector<int64_t> seen((size_t)D, -1);
  for (int64_t t = 0; t < N; t++) {
    int64_t o = X.ptr[t];
    auto put = [&](int64_t col, double x) {
      if (seen[(size_t)col] == t)
        throw Error(MFM_ERR_INVALID, "a row holds the same column twice: sum duplicate entries first (scipy: sum_duplicates)");
      seen[(size_t)col] = t;
      X.idx[(size_t)o] = (int32_t)col;
      X.val[(size_t)o++] = x;
    };
    for (int64_t p = main.ptr[t]; p < main.ptr[t + 1]; p++) put(main.idx[p], main.val[p]);
    for (size_t k = 0; k < blocks.size(); k++) {
      const auto &b = blocks[k];
      const int64_t i = b.map[t];
      for (int64_t p = b.X.ptr[i]; p < b.X.ptr[i + 1]; p++) put(offset[k] + b.X.idx[p], b.X.val[p]);
    }
  }
  Xt = transpose_host(X);
}

mfm_vb::Block vb_make_block(int64_t N, int64_t B, int64_t Db, const int64_t *indptr, const int32_t *indices, const double *data,
                            const int64_t *original_to_block) {
  mfm_vb::Block b;
  b.X = make_host_csr(B, Db, indptr, indices, data);
  b.map.assign(original_to_block, original_to_block + N);
  for (int64_t t = 0; t < N; t++)
    if (b.map[t] < 0 || b.map[t] >= B) throw Error(MFM_ERR_INVALID, "original_to_block out of range");
  return b;
}

// a schedule handed in (mfm_vb_set_levels) must be one the sweeps may run on the LOCAL rows: along every row the levels grow
// with the column index, so no two columns of one level share a row and every column sees the columns before it
int32_t vb_check_levels(const HostCsr &X, const std::vector<int32_t> &level) {
  if ((int64_t)level.size() != X.cols) throw Error(MFM_ERR_INVALID, "mfm_vb_set_levels: one level per column of the expanded design");
  int32_t n_levels = 0;
  for (int32_t l : level) {
    if (l < 0 || l >= X.cols) throw Error(MFM_ERR_INVALID, "mfm_vb_set_levels: a level lies outside [0, D)");
    n_levels = std::max(n_levels, l + 1);
  }
  std::vector<std::pair<int32_t, int32_t>> row;
  for (int64_t t = 0; t < X.rows; t++) {
    row.clear();
    for (int64_t p = X.ptr[t]; p < X.ptr[t + 1]; p++) row.emplace_back(X.idx[p], level[(size_t)X.idx[p]]);
    std::sort(row.begin(), row.end());
    for (size_t k = 1; k < row.size(); k++)
      if (row[k].second <= row[k - 1].second)
        throw Error(MFM_ERR_INVALID, "mfm_vb_set_levels: two columns that share a row must lie in levels that grow with the column index");
  }
  return n_levels;
}
}  // namespace

extern "C" {

int mfm_vb_create(int device, int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices, const double *data,
                  const double *y, mfm_vb **out) {
  *out = nullptr;
  auto *v = new mfm_vb();
  try {
    // (N == 0 is an empty shard once mfm_vb_set_shard has said so; mfm_vb_finalize refuses it otherwise)
    if (N < 0) throw Error(MFM_ERR_INVALID, "the variational trainer needs at least one row");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
      throw Error(MFM_ERR_DEVICE, "no usable HIP device");
    v->device = device;
    v->use();
    MFM_HIP_CHECK(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
    v->N = N;
    v->main = make_host_csr(N, D0, indptr, indices, data);
    v->y_host.assign(y, y + N);
    *out = v;
    return MFM_OK;
  } catch (const Error &ex) {
    g_vb_error = ex.what();
    delete v;
    return ex.code;
  } catch (const std::exception &ex) {
    g_vb_error = ex.what();
    delete v;
    return MFM_ERR_RUNTIME;
  }
}

int mfm_vb_add_block(mfm_vb *v, int64_t B, int64_t Db, const int64_t *indptr, const int32_t *indices, const double *data,
                     const int64_t *original_to_block) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_INVALID, "mfm_vb_add_block after mfm_vb_finalize");
        v->blocks.push_back(vb_make_block(v->N, B, Db, indptr, indices, data, original_to_block));
      },
      false);
}

int mfm_vb_set_stream(mfm_vb *v, void *hip_stream) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_RUNTIME, "mfm_vb_set_stream must be called before mfm_vb_finalize");
        if (v->comm.nccl) throw Error(MFM_ERR_RUNTIME, "mfm_vb_set_stream must be called before mfm_vb_comm_init");
        if (v->own_stream && v->stream) {
          MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
          MFM_HIP_CHECK(hipStreamDestroy(v->stream));
        }
        v->stream = (hipStream_t)hip_stream;
        v->own_stream = false;
        v->comm.stream = v->stream;
      },
      false);
}

int mfm_vb_set_allreduce(mfm_vb *v, int (*fn)(void *user, void *dev_buf, int64_t count), void *user) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_RUNTIME, "mfm_vb_set_allreduce must be called before mfm_vb_finalize");
        v->comm.fn = fn;
        v->comm.user = user;
      },
      false);
}

int mfm_vb_set_shard(mfm_vb *v, int32_t rank, int32_t world, int64_t n_total_rows, int64_t row_offset) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_RUNTIME, "mfm_vb_set_shard must be called before mfm_vb_finalize");
        if (world < 1 || rank < 0 || rank >= world) throw Error(MFM_ERR_INVALID, "bad rank / world size");
        if (n_total_rows < 1 || row_offset < 0 || row_offset + v->N > n_total_rows)
          throw Error(MFM_ERR_INVALID, "the shard's rows [row_offset, row_offset + N) must lie inside n_total_rows >= 1 rows");
        v->comm.rank = rank;
        v->comm.world = world;
        v->comm.shard_set = true;
        v->N_total = n_total_rows;
        v->row_offset = row_offset;
      },
      false);
}

int mfm_vb_comm_init(mfm_vb *v, const void *id128, int32_t rank, int32_t world) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_RUNTIME, "mfm_vb_comm_init must be called before mfm_vb_finalize");
        if (world < 1 || rank < 0 || rank >= world) throw Error(MFM_ERR_INVALID, "bad rank / world size");
        if (v->comm.nccl) throw Error(MFM_ERR_RUNTIME, "communicator already initialised");
        Rccl &r = Rccl::get();
        mfm_nccl_id id;
        std::memcpy(&id, id128, sizeof(id));
        void *comm = nullptr;
        r.check(r.CommInitRank(&comm, world, id, rank), "ncclCommInitRank");
        v->comm.nccl = comm;
        v->comm.stream = v->stream;
        v->comm.rank = rank;
        v->comm.world = world;
      },
      false);
}

int mfm_vb_comm_stats(const mfm_vb *v, int64_t *calls, int64_t *doubles) {
  if (!v) return MFM_ERR_INVALID;
  if (calls) *calls = v->comm.calls;
  if (doubles) *doubles = v->comm.doubles;
  return MFM_OK;
}

int mfm_vb_set_levels(mfm_vb *v, const int32_t *level, int64_t D) {
  return vb_guard(
      v,
      [&]() {
        if (v->finalized) throw Error(MFM_ERR_RUNTIME, "mfm_vb_set_levels must be called before mfm_vb_finalize");
        if (D < 0) throw Error(MFM_ERR_INVALID, "negative number of columns");
        v->given_levels.assign(level, level + D);
      },
      false);
}

int mfm_vb_design_levels(int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices, const double *data,
                         int32_t n_blocks, const int64_t *block_rows, const int64_t *block_cols,
                         const int64_t *const *block_indptr, const int32_t *const *block_indices,
                         const double *const *block_data, const int64_t *const *block_maps, int32_t *level_out,
                         int32_t *n_levels) {
  try {
    if (N < 0 || n_blocks < 0) throw Error(MFM_ERR_INVALID, "negative shape");
    HostCsr main = make_host_csr(N, D0, indptr, indices, data);
    std::vector<mfm_vb::Block> blocks;
    for (int32_t k = 0; k < n_blocks; k++)
      blocks.push_back(vb_make_block(N, block_rows[k], block_cols[k], block_indptr[k], block_indices[k], block_data[k],
                                     block_maps[k]));
    HostCsr X, Xt;
    vb_expand_design(main, blocks, X, Xt);
    std::vector<int32_t> level;
    const int32_t n = column_levels(Xt, level);
    std::copy(level.begin(), level.end(), level_out);
    if (n_levels) *n_levels = n;
    return MFM_OK;
  } catch (const Error &ex) {
    g_vb_error = ex.what();
    return ex.code;
  } catch (const std::exception &ex) {
    g_vb_error = ex.what();
    return MFM_ERR_RUNTIME;
  }
}

int mfm_vb_finalize(mfm_vb *v, const int32_t *group_index, int32_t G, int32_t rank) {
  return vb_guard(
      v,
      [&]() {
    if (v->finalized) throw Error(MFM_ERR_INVALID, "mfm_vb_finalize called twice");
    if (rank < 0) throw Error(MFM_ERR_INVALID, "rank must be non-negative");
    const int64_t N = v->N;
    const bool declared = v->comm.shard_set;
    if (N < 1 && !declared) throw Error(MFM_ERR_INVALID, "the variational trainer needs at least one row");
    if (declared && v->comm.world > 1 && !v->comm.active())
      throw Error(MFM_ERR_INVALID, "a shard of more than one rank needs an all-reduce (mfm_vb_set_allreduce / mfm_vb_comm_init)");
    if (!declared && v->comm.world > 1)
      throw Error(MFM_ERR_INVALID, "a communicator of more than one rank needs mfm_vb_set_shard (n_total_rows, row_offset)");
    if (!declared) v->N_total = N;
    int64_t D = v->main.cols;
    for (auto &b : v->blocks) D += b.X.cols;
    if (G < 0 || (G == 0 && D > 0)) throw Error(MFM_ERR_INVALID, "every feature needs a group");
    HostCsr X, Xt;
    vb_expand_design(v->main, v->blocks, X, Xt);
    v->D = D;
    v->K = rank;
    v->G = G;
    // a shard sees only its own rows: its own schedule could differ from another rank's and the ranks' collectives would not
    // match, so a sharded fit is handed the schedule of the global design
    std::vector<int32_t> level;
    if (!v->given_levels.empty() || (v->sharded() && D > 0 && v->comm.world > 1)) {
      if (v->given_levels.empty()) throw Error(MFM_ERR_INVALID, "a row-sharded fit needs the global level schedule (mfm_vb_set_levels)");
      level = v->given_levels;
      v->n_levels = vb_check_levels(X, level);
    } else {
      v->n_levels = column_levels(Xt, level);
    }
    // columns by (level, index)
    v->level_ptr.assign((size_t)v->n_levels + 1, 0);
    for (int64_t j = 0; j < D; j++) v->level_ptr[(size_t)level[j] + 1]++;
    for (int32_t l = 0; l < v->n_levels; l++) v->level_ptr[l + 1] += v->level_ptr[l];
    v->level_order.resize((size_t)D);
    {
      std::vector<int64_t> cur(v->level_ptr.begin(), v->level_ptr.end() - 1);
      for (int64_t j = 0; j < D; j++) v->level_order[(size_t)cur[level[j]]++] = (int32_t)j;
    }
    // features by group (ascending inside a group)
    std::vector<int64_t> gptr((size_t)G + 1, 0);
    for (int64_t j = 0; j < D; j++) {
      if (group_index[j] < 0 || group_index[j] >= G) throw Error(MFM_ERR_INVALID, "group index out of range");
      gptr[(size_t)group_index[j] + 1]++;
    }
    for (int g = 0; g < G; g++) gptr[g + 1] += gptr[g];
    std::vector<int32_t> gfeat((size_t)D);
    {
      std::vector<int64_t> cur(gptr.begin(), gptr.end() - 1);
      for (int64_t j = 0; j < D; j++) gfeat[(size_t)cur[group_index[j]]++] = (int32_t)j;
    }
    v->ptr.upload(X.ptr);
    v->idx.upload(X.idx);
    v->val.upload(X.val);
    v->cptr.upload(Xt.ptr);
    v->ridx.upload(Xt.idx);
    v->cval.upload(Xt.val);
    v->order.upload(v->level_order);
    v->gptr.upload(gptr);
    v->gfeat.upload(gfeat);
    v->gidx.upload(group_index, (size_t)D);
    v->y.upload(v->y_host);
    const size_t DK = (size_t)D * (size_t)rank;
    v->w.alloc(std::max<size_t>(D, 1));
    v->wv.alloc(std::max<size_t>(D, 1));
    v->V.alloc(std::max<size_t>(DK, 1));
    v->Vv.alloc(std::max<size_t>(DK, 1));
    v->e.alloc((size_t)N);
    v->q.alloc((size_t)N);
    v->x2s.alloc((size_t)N);
    v->x3sv.alloc((size_t)N);
    v->given_levels.clear();
    v->n_parts = (int)std::max<int64_t>(1, std::min<int64_t>(vb::MAX_PARTS, mfm_vb::cdiv_(N, vb::WG)));
    if (v->sharded()) {
      int64_t widest = 1;
      for (int32_t l = 0; l < v->n_levels; l++) widest = std::max(widest, v->level_ptr[l + 1] - v->level_ptr[l]);
      v->S.alloc((size_t)widest * 4);
    }
    v->part.alloc((size_t)v->n_parts * 4);
    v->red.alloc(4);
    v->stats.alloc((size_t)(rank + 1) * G * 3);
    v->hyp.alloc((size_t)(rank + 1) * G * 2);
    v->main = HostCsr();
    v->blocks.clear();
    v->finalized = true;
      },
      false);
}

void mfm_vb_destroy(mfm_vb *v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipStreamSynchronize(v->stream);
  delete v;
}

const char *mfm_vb_last_error(const mfm_vb *v) { return v ? v->err.c_str() : g_vb_error.c_str(); }

int mfm_vb_plan_info(const mfm_vb *v, int64_t *n_levels, int64_t *n_launches_per_iteration) {
  if (!v) return MFM_ERR_INVALID;
  int64_t lv = 0;
  for (int32_t l = 0; l < v->n_levels; l++) lv += v->level_ptr[l + 1] > v->level_ptr[l];
  if (n_levels) *n_levels = v->n_levels;
  // score + reduce, w sweep, per factor the cache and its levels, two group-statistics launches; row-sharded every level is
  // two launches (statistics, apply)
  const int64_t per_level = v->sharded() ? 2 : 1;
  if (n_launches_per_iteration) *n_launches_per_iteration = 2 + per_level * lv + (int64_t)v->K * (1 + per_level * lv) + 2;
  return MFM_OK;
}

int mfm_vb_set_state(mfm_vb *v, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                     const double *V_var) {
  return vb_guard(v, [&]() {
    v->w0 = w0;
    v->w0_var = w0_var;
    const size_t DK = (size_t)v->D * v->K;
    auto put = [&](DevBuf<double> &b, const double *h, size_t n) {
      if (h && n) MFM_HIP_CHECK(hipMemcpy(b.p, h, n * sizeof(double), hipMemcpyHostToDevice));
    };
    put(v->w, w, (size_t)v->D);
    put(v->wv, w_var, (size_t)v->D);
    put(v->V, V, DK);
    put(v->Vv, V_var, DK);
  });
}

int mfm_vb_get_state(mfm_vb *v, double *w0, double *w0_var, double *w, double *w_var, double *V, double *V_var) {
  return vb_guard(v, [&]() {
    MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
    if (w0) *w0 = v->w0;
    if (w0_var) *w0_var = v->w0_var;
    const size_t DK = (size_t)v->D * v->K;
    auto get = [&](double *h, const DevBuf<double> &b, size_t n) {
      if (h && n) MFM_HIP_CHECK(hipMemcpy(h, b.p, n * sizeof(double), hipMemcpyDeviceToHost));
    };
    get(w, v->w, (size_t)v->D);
    get(w_var, v->wv, (size_t)v->D);
    get(V, v->V, DK);
    get(V_var, v->Vv, DK);
  });
}

int mfm_vb_set_w0(mfm_vb *v, double w0, double w0_var) {
  return vb_guard(v, [&]() {
    v->w0 = w0;
    v->w0_var = w0_var;
  });
}

int mfm_vb_update_e(mfm_vb *v, int32_t mode, double *out4) {
  return vb_guard(v, [&]() {
    if (mode != 0 && mode != 1) throw Error(MFM_ERR_INVALID, "mode must be 0 (e -= y) or 1 (classification)");
    hipLaunchKernelGGL(vb::k_vb_score, dim3(v->n_parts), dim3(vb::WG), 0, v->stream, v->N, v->D, v->K, v->ptr.p, v->idx.p,
                       v->val.p, v->w0, v->w.p, v->wv.p, v->V.p, v->Vv.p, v->y.p, (int)mode, v->e.p, v->part.p);
    hipLaunchKernelGGL(vb::k_vb_reduce, dim3(1), dim3(vb::WG), 0, v->stream, v->part.p, v->n_parts, v->red.p);
    MFM_HIP_CHECK(hipGetLastError());
    v->comm.allreduce(v->red.p, 4);  // (row-sharded: the four sums over all ranks' rows as one buffer)
    double h[4];
    MFM_HIP_CHECK(hipMemcpyAsync(h, v->red.p, sizeof(h), hipMemcpyDeviceToHost, v->stream));
    MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
    out4[0] = h[0];
    out4[1] = h[1];
    out4[2] = v->w0_var * (double)v->N_total + h[2];  // (once, after the all-reduce)
    out4[3] = h[3];
  });
}

int mfm_vb_shift_e(mfm_vb *v, double delta) {
  return vb_guard(v, [&]() {
    if (!v->N) return;  // (an empty shard)
    hipLaunchKernelGGL(vb::k_vb_shift, dim3(mfm_vb::cdiv_(v->N, vb::WG)), dim3(vb::WG), 0, v->stream, v->N, v->e.p, delta);
    MFM_HIP_CHECK(hipGetLastError());
  });
}

int mfm_vb_get_e(mfm_vb *v, double *e) {
  return vb_guard(v, [&]() {
    MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
    if (v->N) MFM_HIP_CHECK(hipMemcpy(e, v->e.p, (size_t)v->N * sizeof(double), hipMemcpyDeviceToHost));
  });
}

int mfm_vb_get_cache(mfm_vb *v, double *q, double *x2s, double *x3sv) {
  return vb_guard(v, [&]() {
    MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
    const size_t n = (size_t)v->N * sizeof(double);
    if (!n) return;
    if (q) MFM_HIP_CHECK(hipMemcpy(q, v->q.p, n, hipMemcpyDeviceToHost));
    if (x2s) MFM_HIP_CHECK(hipMemcpy(x2s, v->x2s.p, n, hipMemcpyDeviceToHost));
    if (x3sv) MFM_HIP_CHECK(hipMemcpy(x3sv, v->x3sv.p, n, hipMemcpyDeviceToHost));
  });
}

int mfm_vb_zero_w(mfm_vb *v) {
  return vb_guard(v, [&]() {
    if (v->D) {
      MFM_HIP_CHECK(hipMemsetAsync(v->w.p, 0, (size_t)v->D * sizeof(double), v->stream));
      MFM_HIP_CHECK(hipMemsetAsync(v->wv.p, 0, (size_t)v->D * sizeof(double), v->stream));
    }
  });
}

int mfm_vb_sweep_w(mfm_vb *v, double alpha, const double *lambda_w, const double *mu_w) {
  return vb_guard(v, [&]() {
    v->put_hyp(lambda_w, (size_t)v->G, mu_w, (size_t)v->G);
    const double *lam = v->hyp.p, *mu = v->hyp.p + v->G;
    v->each_level([&](const int32_t *cols, int n, int grid) {
      if (v->sharded()) {
        hipLaunchKernelGGL(vb::k_vb_stats_w, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                           v->w.p, v->e.p, v->S.p);
        v->comm.allreduce(v->S.p, 2 * (int64_t)n);
        hipLaunchKernelGGL(vb::k_vb_apply_w, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                           v->gidx.p, alpha, lam, mu, v->S.p, v->w.p, v->wv.p, v->e.p);
        return;
      }
      hipLaunchKernelGGL(vb::k_vb_sweep_w, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                         v->gidx.p, alpha, lam, mu, v->w.p, v->wv.p, v->e.p);
    });
    MFM_HIP_CHECK(hipGetLastError());
  });
}

int mfm_vb_sweep_V(mfm_vb *v, int32_t f_begin, int32_t f_end, double alpha, const double *lambda_V, const double *mu_V) {
  return vb_guard(v, [&]() {
    if (f_begin < 0 || f_end > v->K || f_begin > f_end) throw Error(MFM_ERR_INVALID, "factor range out of bounds");
    const size_t GK = (size_t)v->G * v->K;
    v->put_hyp(lambda_V, GK, mu_V, GK);
    const int grid_rows = mfm_vb::cdiv_(v->N, vb::WG);
    for (int32_t f = f_begin; f < f_end; f++) {
      double *Vf = v->V.p + (int64_t)f * v->D, *Vvf = v->Vv.p + (int64_t)f * v->D;
      const double *lam = v->hyp.p + (size_t)f * v->G, *mu = v->hyp.p + GK + (size_t)f * v->G;
      if (grid_rows)  // (0: an empty shard)
        hipLaunchKernelGGL(vb::k_vb_cache, dim3(grid_rows), dim3(vb::WG), 0, v->stream, v->N, v->ptr.p, v->idx.p, v->val.p, Vf,
                           Vvf, v->q.p, v->x2s.p, v->x3sv.p);
      v->each_level([&](const int32_t *cols, int n, int grid) {
        if (v->sharded()) {
          hipLaunchKernelGGL(vb::k_vb_stats_v, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                             Vf, Vvf, v->e.p, v->q.p, v->x2s.p, v->x3sv.p, v->S.p);
          v->comm.allreduce(v->S.p, 4 * (int64_t)n);
          hipLaunchKernelGGL(vb::k_vb_apply_v, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                             v->gidx.p, alpha, lam, mu, v->S.p, Vf, Vvf, v->e.p, v->q.p, v->x2s.p, v->x3sv.p);
          return;
        }
        hipLaunchKernelGGL(vb::k_vb_sweep_v, dim3(grid), dim3(vb::WG), 0, v->stream, cols, n, v->cptr.p, v->ridx.p, v->cval.p,
                           v->gidx.p, alpha, lam, mu, Vf, Vvf, v->e.p, v->q.p, v->x2s.p, v->x3sv.p);
      });
    }
    MFM_HIP_CHECK(hipGetLastError());
  });
}

int mfm_vb_group_stats(mfm_vb *v, int32_t s_begin, int32_t s_end, const double *mu, const double *mu_var, double *out) {
  return vb_guard(v, [&]() {
    if (s_begin < 0 || s_end > v->K + 1 || s_begin > s_end) throw Error(MFM_ERR_INVALID, "slot range out of bounds");
    const size_t n = (size_t)(v->K + 1) * v->G;
    v->put_hyp(mu, n, mu_var, n);
    const int blocks = (s_end - s_begin) * v->G;
    if (!blocks) return;
    hipLaunchKernelGGL(vb::k_vb_group_stats, dim3(blocks), dim3(vb::WG), 0, v->stream, v->D, v->G, (int)s_begin, v->gfeat.p,
                       v->gptr.p, v->w.p, v->wv.p, v->V.p, v->Vv.p, v->hyp.p, v->hyp.p + n, v->stats.p);
    MFM_HIP_CHECK(hipGetLastError());
    MFM_HIP_CHECK(hipMemcpyAsync(out, v->stats.p, (size_t)blocks * 3 * sizeof(double), hipMemcpyDeviceToHost, v->stream));
    MFM_HIP_CHECK(hipStreamSynchronize(v->stream));
  });
}

int mfm_vb_synchronize(mfm_vb *v) {
  return vb_guard(v, [&]() { MFM_HIP_CHECK(hipStreamSynchronize(v->stream)); });
}

int mfm_vb_truncated_normal(int32_t right, double mu, double *out3) {
  const VbMoments m = right ? vb_truncnorm_right(mu) : vb_truncnorm_left(mu);
  out3[0] = m.mean;
  out3[1] = m.var;
  out3[2] = m.lnz;
  return MFM_OK;
}

}  // extern "C"
