// mfm_vbmoments.hpp -- posterior mean and variance of the FM score of every design row under the variational estimators' mean-field
// Gaussian posterior: mfm_design_moments_vb. Included by mfm_hip.hip after mfm_predict.hpp.
//
//   E[score]   = w0 + sum x w + 1/2 sum_k (M_k^2 - sum x^2 m^2)                      (the mean model's score)
//   Var[score] = w0_var + sum x^2 wv + sum_k bracket(M, A, B, C, E)_k  (+ extra_var)  (the sums and the bracket: mfm_vb_sums.hpp)
//
// Layout: the prediction path's. (w | V) and (w_var | V_var) are transposed as two "samples" by k_build_vt_batch into row-major
// tables Vt[j][KS] and Vvt[j][KS]; a group of GS lanes takes a row, lane `lig` owns the factor pairs (2 lig, 2 lig + 1), (2 (lig +
// GS), ...) of score_shape, accumulates the five sums and sum x^2 m^2 for them over the row's entries in CSR order, forms its
// factors' share of mean and variance, and the group reduces both with the xor butterfly of k_score / k_score_store. The mean is
// those kernels' score bit for bit (same lane groups, same order of every addition; the rows per group differ, which no row's
// arithmetic sees). No atomics: a rerun is bit-identical.
//
// Relation blocks are never expanded: k_vbm_block tabulates per block row the five sums per factor, the linear mean, the linear
// variance and sum x^2 m^2 (one thread per block row; table rows [5][KS] with the factors innermost, so the gathering group reads
// five contiguous runs), and the row pass adds them in block-list order after the main part, as k_score adds its block caches.
#pragma once
#include "mfm_vb_sums.hpp"

namespace mfm {

struct VbmBlockRef {
  const int32_t *map;                 // [N]: design row -> block row
  const double *T;                    // [B][5][KS]: M, A, B, C, E per factor
  const double *lin, *lv, *ss;        // [B]: sum x w, sum x^2 wv, sum_k sum x^2 m^2
};

struct VbmArgs {
  const double *w, *wv;               // [D]: posterior mean and variance of the linear weights
  const double *vt, *vvt;             // [D][KS]: posterior mean and variance of V, row-major
  double w0, var0;                    // var0 = w0_var + extra_var
  const VbmBlockRef *blk;
  int n_blk, want_prob;
  double *mean, *sd, *prob;           // [N]
};

// one thread per block row m; `off`: the block's first column in the model's feature space
__global__ __launch_bounds__(WG) void k_vbm_block(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                  const double *__restrict__ val, int64_t B, int64_t off, VbmArgs a, int KS,
                                                  double *__restrict__ T, double *__restrict__ lin_out, double *__restrict__ lv_out,
                                                  double *__restrict__ ss_out) {
  const int64_t m = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (m >= B) return;
  const int32_t pb = rowptr[m], pe = rowptr[m + 1];
  double lin = 0.0, lv = 0.0, ss = 0.0;
  for (int32_t p = pb; p < pe; p++) {
    const double x = val[p];
    lin += x * a.w[off + colidx[p]];
    lv += (x * x) * a.wv[off + colidx[p]];
  }
  double *__restrict__ Trow = T + m * 5 * KS;
  for (int f = 0; f < KS; f++) {
    VbSums z;
    for (int32_t p = pb; p < pe; p++) {
      const double x = val[p], x2 = x * x;
      const int64_t j = off + colidx[p];
      const double mu = a.vt[j * KS + f], s = a.vvt[j * KS + f];
      vb_sums_entry(x, x2, mu, s, z.M, z.A, z.B, z.C, z.E);
      ss += x2 * (mu * mu);
    }
    Trow[f] = z.M;
    Trow[KS + f] = z.A;
    Trow[2 * KS + f] = z.B;
    Trow[3 * KS + f] = z.C;
    Trow[4 * KS + f] = z.E;
  }
  lin_out[m] = lin;
  lv_out[m] = lv;
  ss_out[m] = ss;
}

// rows [r0, r1) of the design; rowptr holds absolute positions, a.blk[.].map and the outputs are indexed with the absolute row
template <int GS, int SPL, int RU>
__global__ __launch_bounds__(WG) void k_vbm_rows(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colidx,
                                                 const double *__restrict__ val, VbmArgs a, int K, int KS, int64_t r0, int64_t r1) {
  const int lig = threadIdx.x % GS;
  const int64_t t0 = r0 + (((int64_t)blockIdx.x * WG + threadIdx.x) / GS) * RU;
  double2 M[RU][SPL], A[RU][SPL], B[RU][SPL], C[RU][SPL], E[RU][SPL];
  double b[RU], lin[RU], lv[RU];
  int64_t pb[RU];
  int len[RU];
  int maxlen = 0;
#pragma unroll
  for (int u = 0; u < RU; u++) {
    b[u] = lin[u] = lv[u] = 0.0;
#pragma unroll
    for (int s = 0; s < SPL; s++) M[u][s] = A[u][s] = B[u][s] = C[u][s] = E[u][s] = make_double2(0.0, 0.0);
    const int64_t t = t0 + u;
    if (t < r1) {
      pb[u] = rowptr[t];
      len[u] = rowptr[t + 1] - (int32_t)pb[u];
    } else {
      pb[u] = 0;
      len[u] = 0;
    }
    maxlen = len[u] > maxlen ? len[u] : maxlen;
  }
  for (int k = 0; k < maxlen; k++) {
#pragma unroll
    for (int u = 0; u < RU; u++) {
      if (k < len[u]) {
        const int32_t j = colidx[pb[u] + k];
        const double x = val[pb[u] + k];
        const double x2 = x * x;
        if (lig == 0) {
          lin[u] += x * a.w[j];
          lv[u] += x2 * a.wv[j];
        }
        const double2 *mrow = (const double2 *)(a.vt + (int64_t)j * KS);
        const double2 *srow = (const double2 *)(a.vvt + (int64_t)j * KS);
#pragma unroll
        for (int s = 0; s < SPL; s++) {
          const int pr = lig + s * GS;
          if (2 * pr < K) {
            const double2 v = mrow[pr], sv = srow[pr];  // pad column of an odd K is zero in both tables
            b[u] += x2 * (v.x * v.x);
            b[u] += x2 * (v.y * v.y);
            vb_sums_entry(x, x2, v.x, sv.x, M[u][s].x, A[u][s].x, B[u][s].x, C[u][s].x, E[u][s].x);
            vb_sums_entry(x, x2, v.y, sv.y, M[u][s].y, A[u][s].y, B[u][s].y, C[u][s].y, E[u][s].y);
          }
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RU; u++) {
    const int64_t t = t0 + u;
    if (t < r1) {
      for (int bi = 0; bi < a.n_blk; bi++) {
        const VbmBlockRef &R = a.blk[bi];
        const int64_t i = R.map[t];
        if (lig == 0) {
          lin[u] += R.lin[i];
          lv[u] += R.lv[i];
        }
        const double *row = R.T + i * 5 * KS;
#pragma unroll
        for (int s = 0; s < SPL; s++) {
          const int pr = lig + s * GS;
          if (2 * pr < K) {
            const double2 tm = ((const double2 *)row)[pr], ta = ((const double2 *)(row + KS))[pr],
                          tb = ((const double2 *)(row + 2 * KS))[pr], tc = ((const double2 *)(row + 3 * KS))[pr],
                          te = ((const double2 *)(row + 4 * KS))[pr];
            M[u][s].x += tm.x, M[u][s].y += tm.y;
            A[u][s].x += ta.x, A[u][s].y += ta.y;
            B[u][s].x += tb.x, B[u][s].y += tb.y;
            C[u][s].x += tc.x, C[u][s].y += tc.y;
            E[u][s].x += te.x, E[u][s].y += te.y;
          }
        }
        if (lig == 0) b[u] += R.ss[i];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < RU; u++) {
    double part = 0.0, vpart = 0.0;
#pragma unroll
    for (int s = 0; s < SPL; s++) {
      part += M[u][s].x * M[u][s].x + M[u][s].y * M[u][s].y;
      vpart += vb_bracket(M[u][s].x, A[u][s].x, B[u][s].x, C[u][s].x, E[u][s].x) +
               vb_bracket(M[u][s].y, A[u][s].y, B[u][s].y, C[u][s].y, E[u][s].y);
    }
    part = 0.5 * (part - b[u]) + lin[u];
    vpart += lv[u];
#pragma unroll
    for (int m = GS / 2; m >= 1; m >>= 1) {
      part += __shfl_xor(part, m, WAVE);
      vpart += __shfl_xor(vpart, m, WAVE);
    }
    const int64_t t = t0 + u;
    if (t < r1 && lig == 0) {  // (lane 0's association is the score's, as in k_score)
      const double mean = a.w0 + part;
      const double var = fmax(a.var0 + vpart, 0.0);
      a.mean[t] = mean;
      a.sd[t] = sqrt(var);
      if (a.want_prob) a.prob[t] = (erf(mean / sqrt(1.0 + var) * 0.70710678118654752440) + 1.0) / 2.0;
    }
  }
}

constexpr int64_t VBM_TILE_ROWS = (int64_t)1 << 20;  // rows per launch unless the caller forces a tile

}  // namespace mfm

extern "C" int mfm_design_moments_vb(mfm_design *d, int32_t rank, double w0, double w0_var, const double *w, const double *w_var,
                                     const double *V, const double *V_var, double extra_var, int32_t want_prob, int64_t tile_rows,
                                     double *out_mean, double *out_std, double *out_prob) {
  if (!d) {
    g_global_error = "mfm_design_moments_vb: no design";
    return MFM_ERR_INVALID;
  }
  MFM_TRY(d)
  // (the arguments first: nothing below this block is reached with a bad one, and nothing in it touches the device)
  if (!out_mean || !out_std || (want_prob && !out_prob)) throw Error(MFM_ERR_INVALID, "no output array");
  if (rank < 0) throw Error(MFM_ERR_INVALID, "rank must be non-negative");
  if (rank > 512) throw Error(MFM_ERR_INVALID, "rank > 512 is not supported");
  if (tile_rows < 0) throw Error(MFM_ERR_INVALID, "negative tiling override");
  if (!(extra_var >= 0.0) || !std::isfinite(extra_var)) throw Error(MFM_ERR_INVALID, "extra_var must be finite and non-negative");
  if (!(w0_var >= 0.0)) throw Error(MFM_ERR_INVALID, "w0_var must be non-negative");
  const int64_t N = d->N, D = d->D;
  const int K = rank, KS = (rank + 1) & ~1;
  if (D > 0 && (!w || !w_var || (K > 0 && (!V || !V_var)))) throw Error(MFM_ERR_INVALID, "no posterior arrays");
  if (N == 0) return MFM_OK;
  hipStream_t s = d->stream;

  // (w | V) and (w_var | V_var) as the two "samples" of k_build_vt_batch
  const size_t per = (size_t)D * (size_t)(K + 1);
  DevBuf<double> model, vt, outs;
  model.alloc(std::max<size_t>(2 * per, 1));
  if (D) {
    MFM_HIP_CHECK(hipMemcpy(model.p, w, (size_t)D * sizeof(double), hipMemcpyHostToDevice));
    MFM_HIP_CHECK(hipMemcpy(model.p + per, w_var, (size_t)D * sizeof(double), hipMemcpyHostToDevice));
    if (K) {
      MFM_HIP_CHECK(hipMemcpy(model.p + D, V, (size_t)D * K * sizeof(double), hipMemcpyHostToDevice));
      MFM_HIP_CHECK(hipMemcpy(model.p + per + D, V_var, (size_t)D * K * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  const size_t tab = (size_t)D * (size_t)KS;
  vt.alloc(std::max<size_t>(2 * tab, 1));
  DevBuf<const double *> d_wv;
  d_wv.upload(std::vector<const double *>{model.p, model.p + per});
  if (K > 0 && D > 0) {
    hipLaunchKernelGGL(k_build_vt_batch, dim3((unsigned)cdiv(D, 32), (unsigned)cdiv(KS, 32), 2u), dim3(WG), 0, s,
                       (const double *const *)d_wv.p, D, K, KS, vt.p);
    MFM_HIP_CHECK(hipGetLastError());
  }
  outs.alloc((size_t)N * 3);
  VbmArgs a;
  a.w = model.p;
  a.wv = model.p + per;
  a.vt = vt.p;
  a.vvt = vt.p + tab;
  a.w0 = w0;
  a.var0 = w0_var + extra_var;
  a.blk = nullptr;
  a.n_blk = 0;
  a.want_prob = want_prob ? 1 : 0;
  a.mean = outs.p;
  a.sd = outs.p + N;
  a.prob = outs.p + 2 * N;

  // the blocks' tables, once per call
  std::vector<DevBuf<double>> tables(d->blocks.size());
  std::vector<VbmBlockRef> refs;
  DevBuf<VbmBlockRef> d_refs;
  for (size_t b = 0; b < d->blocks.size(); b++) {
    DevBlock &B = *d->blocks[b];
    const size_t rows = (size_t)B.B;
    tables[b].alloc(std::max<size_t>(rows * (size_t)(5 * KS + 3), 1));
    double *T = tables[b].p, *lin = T + rows * (size_t)(5 * KS);
    refs.push_back(VbmBlockRef{B.map.p, T, lin, lin + rows, lin + 2 * rows});
    if (B.B > 0) {
      hipLaunchKernelGGL(k_vbm_block, dim3((unsigned)cdiv(B.B, WG)), dim3(WG), 0, s, B.X.rowptr.p, B.X.colidx.p, B.X.rval.p, B.B, B.col_off,
                         a, KS, T, lin, lin + rows, lin + 2 * rows);
      MFM_HIP_CHECK(hipGetLastError());
    }
  }
  if (!refs.empty()) {
    d_refs.upload(refs);
    a.blk = d_refs.p;
    a.n_blk = (int)refs.size();
  }

  const int64_t T = tile_rows > 0 ? tile_rows : VBM_TILE_ROWS;
  for (int64_t r0 = 0; r0 < N; r0 += T) {
    const int64_t r1 = std::min(N, r0 + T);
    (void)score_shape(K, d->X, [&](auto gs, auto spl, auto, auto) {
      constexpr int GS = decltype(gs)::value, SPL = decltype(spl)::value;
      constexpr int RU = SPL == 1 ? 2 : 1;  // (20 SPL registers of sums per row in flight)
      const int64_t groups = (r1 - r0 + RU - 1) / RU;
      hipLaunchKernelGGL((k_vbm_rows<GS, SPL, RU>), dim3((unsigned)cdiv(groups * GS, WG)), dim3(WG), 0, s, d->X.rowptr.p, d->X.colidx.p,
                         d->X.rval.p, a, K, KS, r0, r1);
    });
    MFM_HIP_CHECK(hipGetLastError());
  }
  MFM_HIP_CHECK(hipMemcpyAsync(out_mean, outs.p, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipMemcpyAsync(out_std, outs.p + N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  if (want_prob) MFM_HIP_CHECK(hipMemcpyAsync(out_prob, outs.p + 2 * N, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipStreamSynchronize(s));
  MFM_CATCH(d)
}
