// mfm_foldin_gibbs.hip -- mfm_foldin_gibbs_*: the parameters of new one-hot features under every kept sample of a probit model
// (classifier or ordered probit), by a short Albert-Chib chain per (entity, sample) on chip (kernel and algebra:
// mfm_foldin_gibbs.hpp). The handle is mfm_foldin_create's, its y the labels.
//
// Memory rule. Unlike the closed form of mfm_foldin.hip a chain reads every row's z and f once per sweep, so a cell keeps them in
// device scratch: n_u (M + 1) doubles, next to its result. The call walks the entities in chunks whose scratch stays under the
// handle's bound (mfm_foldin_gibbs_plan.hpp: chunk edges from the prefix sums of the entity offsets; below one entity's worth the
// samples are walked; a single cell larger than the bound runs alone). A result does not depend on the chunking.
#include "mfm_foldin_gibbs.hpp"
#include "mfm_foldin_handle.hpp"
#include "mfm_samples.hpp"

using namespace mfm;

namespace {

template <int TASK, bool DRAW>
void launch_foldin_gibbs(hipStream_t s, dim3 grid, size_t lds, const FoldinGibbsArgs &a) {
  static DeviceOnce raised;
  if (raised.need()) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k_foldin_gibbs<TASK, DRAW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)foldin_lds_bytes(FOLDIN_MAX_RANK + 1)));
    raised.mark();
  }
  hipLaunchKernelGGL((k_foldin_gibbs<TASK, DRAW>), grid, dim3(FOLDIN_WG), lds, s, a);
}

// The whole call over the samples of `v`: w_new[S][U], V_new[S][U][K].
void run_foldin_gibbs(mfm_foldin *p, const SampleView &v, int task, int n_class, const double *cut, const double *mu, const double *lam,
                      int n_burn, int n_inner, int draw, uint64_t seed, double *w_new, double *V_new) {
  const int S = v.count(), K = v.K;
  if (v.device != p->device) throw Error(MFM_ERR_INVALID, "fold-in observations and sample store live on different devices");
  if (v.D != p->D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  if (K > FOLDIN_MAX_RANK)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(FOLDIN_MAX_RANK) + ", the samples have rank " + std::to_string(K));
  if (S > 65535) throw Error(MFM_ERR_INVALID, "at most 65535 samples per call");
  if (!w_new || (K > 0 && !V_new)) throw Error(MFM_ERR_INVALID, "no output array");
  const int off = p->lin ? 1 : 0, M = K + off;
  const std::string refusal = foldin_gibbs_check(S, K, off, task, n_class, cut, mu, lam, n_burn, n_inner, p->h_y.data(), p->n);
  if (!refusal.empty()) throw Error(MFM_ERR_INVALID, refusal);
  const int64_t U = p->U;
  if (U == 0 || S == 0) return;
  if (M == 0) {  // rank 0 without a linear term: nothing to estimate
    std::fill(w_new, w_new + (size_t)S * U, 0.0);
    return;
  }
  hipStream_t st = p->stream;
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(st, v.pushed, 0));

  const int64_t *eoff = p->h_eoff.data();
  const std::vector<FoldinChunk> chunks = foldin_gibbs_plan(eoff, U, S, M, K, p->scratch_bound);
  size_t zf_max = 1, cells_max = 1;
  for (const FoldinChunk &c : chunks) {
    zf_max = std::max(zf_max, (size_t)c.ns * (size_t)(eoff[c.u0 + c.nu] - eoff[c.u0]) * (size_t)(M + 1));
    cells_max = std::max(cells_max, (size_t)c.ns * (size_t)c.nu);
  }

  DevBuf<const double *> d_wv;
  DevBuf<double> d_w0, d_mu, d_lam, d_cut, zf, ow, oV;
  DevBuf<int> d_err;
  d_wv.upload(v.wv);
  d_w0.upload(v.w0);
  d_mu.upload(mu, (size_t)S * (K + 1));
  d_lam.upload(lam, (size_t)S * (K + 1));
  if (task == FOLDIN_TASK_ORDERED) d_cut.upload(cut, (size_t)S * (n_class - 1));
  d_err.alloc_zero(1, st);
  zf.alloc(zf_max);
  ow.alloc(cells_max);
  oV.alloc(std::max<size_t>(cells_max * K, 1));

  FoldinGibbsArgs g;
  FoldinArgs &a = g.a;
  a.rowptr = p->ptr.p;
  a.colidx = p->idx.p;
  a.val = p->val.p;
  a.y = p->y.p;
  a.eoff = p->eoff.p;
  a.wv = (const double *const *)d_wv.p;
  a.w0 = d_w0.p;
  a.alpha = nullptr;
  a.mu = d_mu.p;
  a.lam = d_lam.p;
  a.D = p->D;
  a.U = U;
  a.K = K;
  a.lin = off;
  a.seed = seed;
  a.out_w = ow.p;
  a.out_V = oV.p;
  a.err = d_err.p;
  g.cut = d_cut.p;
  g.n_class = n_class;
  g.n_burn = n_burn;
  g.n_inner = n_inner;
  g.n = p->n;
  g.zf = zf.p;
  const size_t lds = foldin_lds_bytes(M);
  for (const FoldinChunk &c : chunks) {
    a.u0 = c.u0;
    a.s0 = c.s0;
    g.rows = eoff[c.u0 + c.nu] - eoff[c.u0];
    const dim3 grid((unsigned)c.nu, (unsigned)c.ns);
    if (task == FOLDIN_TASK_ORDERED) {
      if (draw)
        launch_foldin_gibbs<FOLDIN_TASK_ORDERED, true>(st, grid, lds, g);
      else
        launch_foldin_gibbs<FOLDIN_TASK_ORDERED, false>(st, grid, lds, g);
    } else {
      if (draw)
        launch_foldin_gibbs<FOLDIN_TASK_CLASSIFIER, true>(st, grid, lds, g);
      else
        launch_foldin_gibbs<FOLDIN_TASK_CLASSIFIER, false>(st, grid, lds, g);
    }
    MFM_HIP_CHECK(hipGetLastError());
    // the chunk's rows [ns][nu] into w_new[S][U] at (s0, u0), [ns][nu * K] into V_new[S][U * K] at (s0, u0 * K)
    MFM_HIP_CHECK(hipMemcpy2DAsync(w_new + (size_t)c.s0 * U + c.u0, (size_t)U * sizeof(double), ow.p, (size_t)c.nu * sizeof(double),
                                   (size_t)c.nu * sizeof(double), (size_t)c.ns, hipMemcpyDeviceToHost, st));
    if (K > 0)
      MFM_HIP_CHECK(hipMemcpy2DAsync(V_new + ((size_t)c.s0 * U + c.u0) * K, (size_t)U * K * sizeof(double), oV.p,
                                     (size_t)c.nu * K * sizeof(double), (size_t)c.nu * K * sizeof(double), (size_t)c.ns,
                                     hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipStreamSynchronize(st));
  }
  int h_err = 0;
  MFM_HIP_CHECK(hipMemcpyAsync(&h_err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  MFM_HIP_CHECK(hipStreamSynchronize(st));
  if (h_err)
    throw Error(MFM_ERR_INVALID, "fold-in: a posterior precision matrix is not positive definite or a row's score is not finite (a "
                                 "non-finite model value); no result is returned");
}

}  // namespace

extern "C" {

int mfm_foldin_gibbs_solve_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, int32_t task, int32_t n_class,
                                 const double *cutpoints, const double *mu, const double *lambda, int32_t n_burn, int32_t n_inner,
                                 int32_t draw, uint64_t seed, double *w_new, double *V_new) {
  FOLDIN_TRY(p)
  if (!st) throw Error(MFM_ERR_INVALID, "no sample store");
  run_foldin_gibbs(p, samples_of_store(st, first, count), task, n_class, cutpoints, mu, lambda, n_burn, n_inner, draw, seed, w_new, V_new);
  FOLDIN_CATCH(p)
}

int mfm_foldin_gibbs_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t task, int32_t n_class, const double *cutpoints, const double *mu, const double *lambda,
                           int32_t n_burn, int32_t n_inner, int32_t draw, uint64_t seed, double *w_new, double *V_new) {
  FOLDIN_TRY(p)
  if (rank > FOLDIN_MAX_RANK)  // (before the samples are uploaded)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(FOLDIN_MAX_RANK) + ", the samples have rank " + std::to_string(rank));
  run_foldin_gibbs(p, samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs), task, n_class, cutpoints, mu, lambda, n_burn,
                   n_inner, draw, seed, w_new, V_new);
  FOLDIN_CATCH(p)
}

}  // extern "C"
