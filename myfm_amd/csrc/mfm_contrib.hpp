// mfm_contrib.hpp -- the score of every kept sample taken apart by field (not in the reference). With field_of[j] in
// [0, F) for every column j of the flat design (main columns, then the relation blocks'), one row x and one sample s:
//   p_g[k] = sum_{j in g} x_j V_s[k, j]      q_g = sum_{j in g} x_j^2 sum_k V_s[k, j]^2      lin_g = sum_{j in g} x_j w_s[j]
//   I_gg = (sum_k p_g[k]^2 - q_g) / 2        I_gh = sum_k p_g[k] p_h[k] (g < h)              score_s = w0_s + sum lin + sum I
// and per row and component the mean and the population standard deviation over the samples, in sample order. Components: the F
// linear terms, then the P = F (F + 1) / 2 interactions at the packed index g F - g (g - 1) / 2 + (h - g), g <= h.
// Included by mfm_hip.hip after mfm_dist.hpp (check_tiling, check_sample_source and the staged samples of mfm_predict.hpp).
//
// k_contrib is a row pass at the level of k_score_store: a group of GS lanes per row, ONE factor per lane (factor k of a chunk of GS
// factors is lane k's; rank > GS walks the row once per chunk), the samples the inner loop over the staged row-major V copies.
// An entry's field is a runtime value: the F accumulators p_g, q_g, lin_g are selected by compile-time g (a compare and a select
// per field and entry), never indexed, so an interleaved grouping costs what a contiguous one does. Every component is reduced
// over the group by an xor butterfly (the same bits in every lane, whatever the group's place in the wavefront); component c
// of the bucket belongs to lane c % GS, which keeps the sample's value, the streaming mean and M2 of its ceil(C / GS) components
// in registers under compile-time slot numbers. No LDS, no atomics; between sample chunks mean and M2 travel through the output
// buffers, so the chunk does not change a bit. Relation blocks are walked in place through their row maps (no expansion, no
// table per block row: see DESIGN for why).
#pragma once
#include <utility>

namespace mfm {

constexpr int CONTRIB_MAX_FIELDS = 16;

// ---- one (row, sample)'s arithmetic, the same text on the device and in contrib_row_host ----
// an entry (field f, value x) against the lane's factor value v: into the field's p and q
template <int FB>
__host__ __device__ __forceinline__ void contrib_entry(int f, double x, double v, double *p, double *q) {
#pragma clang fp contract(off)
  const double xv = x * v, x2v2 = (x * x) * (v * v);
#pragma unroll
  for (int g = 0; g < FB; g++) {
    p[g] = f == g ? p[g] + xv : p[g];
    q[g] = f == g ? q[g] + x2v2 : q[g];
  }
}
template <int FB>
__host__ __device__ __forceinline__ void contrib_entry_lin(int f, double x, double wj, double *lin) {
#pragma clang fp contract(off)
  const double xw = x * wj;
#pragma unroll
  for (int g = 0; g < FB; g++) lin[g] = f == g ? lin[g] + xw : lin[g];
}
// a lane's part of I_gh; a field of one unit entry: p = v, q = v v, the difference exactly 0
__host__ __device__ __forceinline__ double contrib_pair_part(bool same, double pg, double ph, double qg) {
#pragma clang fp contract(off)
  const double pp = pg * ph;
  return same ? 0.5 * (pp - qg) : pp;
}
// value x as the n-th of the stream, rn = 1 / n: equal values leave M2 exactly 0
__host__ __device__ __forceinline__ void contrib_moment(double x, double rn, double &mean, double &m2) {
#pragma clang fp contract(off)
  const double delta = x - mean;
  mean = mean + delta * rn;
  m2 = m2 + delta * (x - mean);
}
__host__ __device__ __forceinline__ double contrib_std(double m2, int n) { return sqrt(m2 / (double)n); }

// the packed pair (g, h), g <= h, of F fields, and back
__host__ __device__ constexpr int contrib_pair_index(int F, int g, int h) { return g * F - g * (g - 1) / 2 + (h - g); }
__host__ __device__ constexpr int contrib_pair_g(int F, int idx) {
  int g = 0;
  while (idx >= F - g) {
    idx -= F - g;
    g++;
  }
  return g;
}
__host__ __device__ constexpr int contrib_pair_h(int F, int idx) {
  int g = 0;
  while (idx >= F - g) {
    idx -= F - g;
    g++;
  }
  return g + idx;
}

// The shapes. Buckets of fields FB in {2, 4, 8, 16}; lanes per row GS in {4, 16, 32, 64} by rank, and at least 16 for FB = 16 so
// that a lane keeps at most 10 components (the listing).
static int contrib_bucket(int F) { return F <= 2 ? 2 : F <= 4 ? 4 : F <= 8 ? 8 : 16; }
static int contrib_group(int K, int FB) {
  const int gs = K <= 4 ? 4 : K <= 16 ? 16 : K <= 32 ? 32 : 64;
  return FB == 16 && gs < 16 ? 16 : gs;
}

template <class Fn, int... I>
__device__ __forceinline__ void contrib_static_for(const Fn &fn, std::integer_sequence<int, I...>) {
  (fn(std::integral_constant<int, I>{}), ...);
}

// one source of a row's entries: the main matrix (map null: row t), or a relation block (row map[t], columns from col_off)
struct ContribSeg {
  const int32_t *rowptr, *colidx;
  const double *val;
  const int32_t *map;
  int64_t col_off;
};
struct ContribArgs {
  const ContribSeg *segs;
  const int32_t *field_of;  // [D]
  const double *const *wv;  // [S] the chunk's sample buffers (w then V)
  const double *vt_all;     // [S][D][KS]
  double *mean, *m2;        // [F + P][ld]; m2 holds the standard deviation after the last chunk
  int64_t D, ld, r0, Tn;
  int n_seg, S, K, KS, F;
  int s0, total;            // the chunk's first sample among all `total`
};

template <int FB, int GS>
__global__ __launch_bounds__(WG) void k_contrib(ContribArgs a) {
  constexpr int CB = FB + FB * (FB + 1) / 2;  // components of the bucket
  constexpr int SL = (CB + GS - 1) / GS;      // ... per lane
  const int lig = threadIdx.x % GS;
  const int64_t gi = ((int64_t)blockIdx.x * WG + threadIdx.x) / GS;
  if (gi >= a.Tn) return;  // (a whole group leaves)
  const int64_t t = a.r0 + gi;
  const int F = a.F, K = a.K, KS = a.KS;
  // where bucket component CBI lies in the outputs (-1: not a component of F fields)
  const auto out_index = [&](auto cbi) -> int {
    constexpr int c = decltype(cbi)::value;
    if constexpr (c < FB) {
      return c < F ? c : -1;
    } else {
      constexpr int g = contrib_pair_g(FB, c - FB), h = contrib_pair_h(FB, c - FB);
      return h < F ? F + contrib_pair_index(F, g, h) : -1;
    }
  };
  double cur[SL], mean[SL], m2[SL];
#pragma unroll
  for (int i = 0; i < SL; i++) cur[i] = mean[i] = m2[i] = 0.0;
  if (a.s0 > 0)
    contrib_static_for(
        [&](auto cbi) {
          constexpr int c = decltype(cbi)::value;
          const int o = out_index(cbi);
          if (lig == c % GS && o >= 0) {
            mean[c / GS] = a.mean[(size_t)o * a.ld + t];
            m2[c / GS] = a.m2[(size_t)o * a.ld + t];
          }
        },
        std::make_integer_sequence<int, CB>{});
  for (int smp = 0; smp < a.S; smp++) {
    const double *__restrict__ Vt = a.vt_all + (size_t)smp * a.D * KS;
    const double *__restrict__ w = a.wv[smp];
    for (int kc = 0; kc == 0 || kc < K; kc += GS) {
      const int k = kc + lig;
      const bool has = k < K;
      double p[FB], q[FB], lin[FB];
#pragma unroll
      for (int g = 0; g < FB; g++) p[g] = q[g] = lin[g] = 0.0;
      for (int sg = 0; sg < a.n_seg; sg++) {
        const ContribSeg seg = a.segs[sg];
        const int64_t row = seg.map ? (int64_t)seg.map[t] : t;
        const int32_t e0 = seg.rowptr[row], e1 = seg.rowptr[row + 1];
        for (int32_t e = e0; e < e1; e++) {
          const int64_t j = seg.col_off + seg.colidx[e];
          const double x = seg.val[e];
          const int f = a.field_of[j];
          const double v = has ? Vt[j * KS + k] : 0.0;
          contrib_entry<FB>(f, x, v, p, q);
          if (kc == 0) contrib_entry_lin<FB>(f, x, w[j], lin);
        }
      }
      contrib_static_for(
          [&](auto cbi) {
            constexpr int c = decltype(cbi)::value;
            if constexpr (c < FB) {
              // a linear term: the same in every lane, taken with the first factor chunk
              if (kc == 0 && lig == c % GS) cur[c / GS] = lin[c];
            } else {
              constexpr int g = contrib_pair_g(FB, c - FB), h = contrib_pair_h(FB, c - FB);
              if (h < F) {  // (uniform)
                double part = contrib_pair_part(g == h, p[g], p[h], q[g]);
#pragma unroll
                for (int m = GS / 2; m >= 1; m >>= 1) part += __shfl_xor(part, m, WAVE);
                if (lig == c % GS) cur[c / GS] = kc == 0 ? part : cur[c / GS] + part;
              }
            }
          },
          std::make_integer_sequence<int, CB>{});
    }
    const double rn = 1.0 / (double)(a.s0 + smp + 1);
#pragma unroll
    for (int i = 0; i < SL; i++) contrib_moment(cur[i], rn, mean[i], m2[i]);
  }
  const bool last = a.s0 + a.S == a.total;
  contrib_static_for(
      [&](auto cbi) {
        constexpr int c = decltype(cbi)::value;
        const int o = out_index(cbi);
        if (lig == c % GS && o >= 0) {
          a.mean[(size_t)o * a.ld + t] = mean[c / GS];
          a.m2[(size_t)o * a.ld + t] = last ? contrib_std(m2[c / GS], a.total) : m2[c / GS];
        }
      },
      std::make_integer_sequence<int, CB>{});
}

static void launch_contrib(hipStream_t s, const ContribArgs &a) {
  const int FB = contrib_bucket(a.F), GS = contrib_group(a.K, FB);
  const dim3 grid((unsigned)cdiv(a.Tn * GS, WG)), block(WG);
#define MFM_CONTRIB(FB_, GS_)                                             \
  if (FB == FB_ && GS == GS_) {                                           \
    hipLaunchKernelGGL((k_contrib<FB_, GS_>), grid, block, 0, s, a); \
    return;                                                               \
  }
  MFM_CONTRIB(2, 4);
  MFM_CONTRIB(2, 16);
  MFM_CONTRIB(2, 32);
  MFM_CONTRIB(2, 64);
  MFM_CONTRIB(4, 4);
  MFM_CONTRIB(4, 16);
  MFM_CONTRIB(4, 32);
  MFM_CONTRIB(4, 64);
  MFM_CONTRIB(8, 4);
  MFM_CONTRIB(8, 16);
  MFM_CONTRIB(8, 32);
  MFM_CONTRIB(8, 64);
  MFM_CONTRIB(16, 16);
  MFM_CONTRIB(16, 32);
  MFM_CONTRIB(16, 64);
#undef MFM_CONTRIB
  throw Error(MFM_ERR_RUNTIME, "no contribution kernel for this shape");
}

// One row on the host in the kernel's orders: the lanes of its group one after the other, the butterfly as the lanes run it.
// idx / val: the row's n entries in the flat design, in the order the kernel meets them (main matrix, then block by block);
// ws[S][D], Vs[S][K][D]; out_mean / out_std [F + P].
template <int FB>
static void contrib_row_host(int GS, int n, const int32_t *idx, const double *val, int64_t D, int K, int S, const double *ws,
                             const double *Vs, int F, const int32_t *field_of, double *out_mean, double *out_std) {
  constexpr int PB = FB * (FB + 1) / 2;
  const int C = F + F * (F + 1) / 2;
  std::vector<double> mean((size_t)C, 0.0), m2((size_t)C, 0.0), cur((size_t)C, 0.0), part((size_t)GS);
  std::vector<double> p((size_t)GS * FB), q((size_t)GS * FB);
  for (int s = 0; s < S; s++) {
    const double *w = ws + (size_t)s * D, *V = Vs + (size_t)s * K * D;
    for (int kc = 0; kc == 0 || kc < K; kc += GS) {
      double lin[FB];
      for (int g = 0; g < FB; g++) lin[g] = 0.0;
      std::fill(p.begin(), p.end(), 0.0);
      std::fill(q.begin(), q.end(), 0.0);
      for (int l = 0; l < GS; l++) {
        const int k = kc + l;
        for (int e = 0; e < n; e++) {
          const int64_t j = idx[e];
          const double v = k < K ? V[(size_t)k * D + j] : 0.0;
          contrib_entry<FB>(field_of[j], val[e], v, &p[(size_t)l * FB], &q[(size_t)l * FB]);
          if (kc == 0 && l == 0) contrib_entry_lin<FB>(field_of[j], val[e], w[j], lin);
        }
      }
      if (kc == 0)
        for (int g = 0; g < F; g++) cur[(size_t)g] = lin[g];
      for (int c = 0; c < PB; c++) {
        const int g = contrib_pair_g(FB, c), h = contrib_pair_h(FB, c);
        if (h >= F) continue;
        for (int l = 0; l < GS; l++) part[(size_t)l] = contrib_pair_part(g == h, p[(size_t)l * FB + g], p[(size_t)l * FB + h], q[(size_t)l * FB + g]);
        for (int m = GS / 2; m >= 1; m >>= 1) {
          std::vector<double> nx((size_t)GS);
          for (int l = 0; l < GS; l++) nx[(size_t)l] = part[(size_t)l] + part[(size_t)(l ^ m)];
          part.swap(nx);
        }
        const size_t o = (size_t)F + (size_t)contrib_pair_index(F, g, h);
        cur[o] = kc == 0 ? part[0] : cur[o] + part[0];
      }
    }
    const double rn = 1.0 / (double)(s + 1);
    for (int c = 0; c < C; c++) contrib_moment(cur[(size_t)c], rn, mean[(size_t)c], m2[(size_t)c]);
  }
  for (int c = 0; c < C; c++) {
    out_mean[c] = mean[(size_t)c];
    out_std[c] = contrib_std(m2[(size_t)c], S);
  }
}

// Every argument check of a call; nothing here touches the device.
static void contrib_check(int64_t D, int32_t n_fields, const int32_t *field_of, int64_t n_field_of, int64_t tile_rows, int32_t chunk_samples) {
  if (n_fields < 1 || n_fields > CONTRIB_MAX_FIELDS)
    throw Error(MFM_ERR_INVALID, "the number of fields must lie in [1, " + std::to_string(CONTRIB_MAX_FIELDS) + "], got " + std::to_string(n_fields));
  if (n_field_of != D)
    throw Error(MFM_ERR_INVALID, "field_of holds one field per column of the design: " + std::to_string(D) + " expected, got " + std::to_string(n_field_of));
  if (D > 0 && !field_of) throw Error(MFM_ERR_INVALID, "field_of is missing");
  for (int64_t j = 0; j < D; j++)
    if (field_of[j] < 0 || field_of[j] >= n_fields)
      throw Error(MFM_ERR_INVALID, "field_of[" + std::to_string(j) + "] = " + std::to_string(field_of[j]) + " lies outside [0, " + std::to_string(n_fields) + ")");
  check_tiling(tile_rows, chunk_samples);
}

struct ContribOut {
  double *bias;  // [2] mean and standard deviation of w0
  double *linear, *linear_std, *interaction, *interaction_std;  // (F, N), (F, N), (P, N), (P, N)
};

static void design_contrib(mfm_design *d, const SampleView &v, int32_t F, const int32_t *field_of, int64_t tile_rows, int32_t chunk_samples,
                           const ContribOut &out) {
  const int count = v.count();
  check_sample_source(d, v);
  {  // w0 over the samples, by the recurrence of the rows
    double mean = 0.0, m2 = 0.0;
    for (int k = 0; k < count; k++) contrib_moment(v.w0[(size_t)k], 1.0 / (double)(k + 1), mean, m2);
    out.bias[0] = mean;
    out.bias[1] = contrib_std(m2, count);
  }
  const int64_t N = d->N, D = d->D;
  if (N == 0) return;
  hipStream_t s = d->stream;
  const size_t P = (size_t)F * ((size_t)F + 1) / 2, C = (size_t)F + P, n = (size_t)N;
  design_use_rank(d, v.K, s);
  if (d->dist_out.n < 2 * C * n) d->dist_out.alloc(2 * C * n);
  d->contrib_field.upload(field_of, (size_t)D);
  std::vector<ContribSeg> segs;
  segs.push_back(ContribSeg{d->X.rowptr.p, d->X.colidx.p, d->X.rval.p, nullptr, 0});
  for (const auto &B : d->blocks) segs.push_back(ContribSeg{B->X.rowptr.p, B->X.colidx.p, B->X.rval.p, B->map.p, B->col_off});
  static_assert(sizeof(ContribSeg) % sizeof(int64_t) == 0, "the segments are uploaded as 64-bit words");
  d->contrib_segs.upload((const int64_t *)segs.data(), segs.size() * sizeof(ContribSeg) / sizeof(int64_t));
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(s, v.pushed, 0));
  const int chunk = design_stage_samples(d, s, v, chunk_samples);
  const int64_t T = tile_rows > 0 ? std::min<int64_t>(tile_rows, N) : N;
  ContribArgs a;
  std::memset(&a, 0, sizeof(a));
  a.segs = (const ContribSeg *)d->contrib_segs.p;
  a.n_seg = (int)segs.size();
  a.field_of = d->contrib_field.p;
  a.mean = d->dist_out.p;
  a.m2 = d->dist_out.p + C * n;
  a.D = D;
  a.ld = N;
  a.K = v.K;
  a.KS = d->KS;
  a.F = F;
  a.total = count;
  for (int c0 = 0; c0 < count; c0 += chunk) {
    const int Cn = std::min(chunk, count - c0);
    const ScoreStoreArgs sa = design_sample_chunk(d, s, c0, Cn, true);
    a.wv = sa.wv;
    a.vt_all = sa.vt_all;
    a.S = Cn;
    a.s0 = c0;
    for (int64_t r0 = 0; r0 < N; r0 += T) {
      a.r0 = r0;
      a.Tn = std::min<int64_t>(T, N - r0);
      launch_contrib(s, a);
    }
    MFM_HIP_CHECK(hipGetLastError());
  }
  const size_t Fn = (size_t)F * n, Pn = P * n;
  MFM_HIP_CHECK(hipMemcpyAsync(out.linear, d->dist_out.p, Fn * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipMemcpyAsync(out.interaction, d->dist_out.p + Fn, Pn * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipMemcpyAsync(out.linear_std, d->dist_out.p + C * n, Fn * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipMemcpyAsync(out.interaction_std, d->dist_out.p + C * n + Fn, Pn * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

static void contrib_check_out(const ContribOut &o) {
  if (!o.bias || !o.linear || !o.linear_std || !o.interaction || !o.interaction_std) throw Error(MFM_ERR_INVALID, "an output array is missing");
}

}  // namespace mfm

extern "C" {

int mfm_design_contrib_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t n_fields, const int32_t *field_of,
                             int64_t n_field_of, int64_t tile_rows, int32_t chunk_samples, double *out_bias, double *out_linear,
                             double *out_linear_std, double *out_interaction, double *out_interaction_std) {
  MFM_TRY(d)
  const mfm::ContribOut out{out_bias, out_linear, out_linear_std, out_interaction, out_interaction_std};
  mfm::contrib_check(d->D, n_fields, field_of, n_field_of, tile_rows, chunk_samples);
  mfm::contrib_check_out(out);
  mfm::design_contrib(d, samples_of_store(st, first, count), n_fields, field_of, tile_rows, chunk_samples, out);
  MFM_CATCH(d)
}

// host samples: checked, then all S uploaded for this call under the rule of mfm_design_summary
int mfm_design_contrib(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t n_fields, const int32_t *field_of, int64_t n_field_of, int64_t tile_rows, int32_t chunk_samples,
                       double *out_bias, double *out_linear, double *out_linear_std, double *out_interaction, double *out_interaction_std) {
  MFM_TRY(d)
  const mfm::ContribOut out{out_bias, out_linear, out_linear_std, out_interaction, out_interaction_std};
  mfm::contrib_check(d->D, n_fields, field_of, n_field_of, tile_rows, chunk_samples);
  mfm::contrib_check_out(out);
  store_check_fraction(d->D, rank, n_samples);
  mfm::design_contrib(d, samples_of_host(d->device, d->D, rank, n_samples, w0s, ws, Vs), n_fields, field_of, tile_rows, chunk_samples, out);
  MFM_CATCH(d)
}

// one row on the host, by the functions the kernel runs and in its orders (no device)
int mfm_contrib_row(int32_t n, const int32_t *idx, const double *val, int64_t D, int32_t rank, int32_t S, const double *ws, const double *Vs,
                    int32_t n_fields, const int32_t *field_of, int64_t n_field_of, double *out_mean, double *out_std) {
  try {
    mfm::contrib_check(D, n_fields, field_of, n_field_of, 0, 0);
    if (n < 0 || rank < 0 || S < 1 || !out_mean || !out_std) throw mfm::Error(MFM_ERR_INVALID, "a row, a rank, at least one sample and the two outputs are needed");
    for (int e = 0; e < n; e++)
      if (idx[e] < 0 || idx[e] >= D) throw mfm::Error(MFM_ERR_INVALID, "column index out of range");
    const int FB = mfm::contrib_bucket(n_fields), GS = mfm::contrib_group(rank, FB);
    if (FB == 2)
      mfm::contrib_row_host<2>(GS, n, idx, val, D, rank, S, ws, Vs, n_fields, field_of, out_mean, out_std);
    else if (FB == 4)
      mfm::contrib_row_host<4>(GS, n, idx, val, D, rank, S, ws, Vs, n_fields, field_of, out_mean, out_std);
    else if (FB == 8)
      mfm::contrib_row_host<8>(GS, n, idx, val, D, rank, S, ws, Vs, n_fields, field_of, out_mean, out_std);
    else
      mfm::contrib_row_host<16>(GS, n, idx, val, D, rank, S, ws, Vs, n_fields, field_of, out_mean, out_std);
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
