// mfm_foldin.hip -- mfm_foldin_*: the parameters of new one-hot features (users or items that were not in the training table) under
// every kept sample, from a few observations of each: one (K + 1)-dimensional Gaussian posterior per (entity, sample), its mean or a
// draw from it (kernel and algebra: mfm_foldin.hpp).
//
// Memory rule. The observations (context rows, targets, entity offsets) are resident for the handle's life. Nothing per row is
// written to device memory: a workgroup keeps its pass of rows in LDS. The only scratch is the result itself, (K + 1) doubles per
// (entity, sample); the call walks the entities -- and, where one entity's samples alone exceed the bound, the samples -- in chunks
// whose results stay under `scratch_bound` bytes (256 MB unless mfm_foldin_set_scratch_bound says otherwise; never less than one
// (entity, sample)). A result does not depend on the chunking.
#include "mfm_foldin.hpp"
#include "mfm_foldin_handle.hpp"
#include "mfm_samples.hpp"

#include <cmath>
#include <memory>

using namespace mfm;

static thread_local std::string g_foldin_error;

namespace {

template <bool DRAW>
void launch_foldin(hipStream_t s, dim3 grid, size_t lds, const FoldinArgs &a) {
  static DeviceOnce raised;
  if (raised.need()) {  // (the largest form once: rank 64 asks for 77 KB)
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k_foldin<DRAW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)foldin_lds_bytes(FOLDIN_MAX_RANK + 1)));
    raised.mark();
  }
  hipLaunchKernelGGL((k_foldin<DRAW>), grid, dim3(FOLDIN_WG), lds, s, a);
}

// The whole call over the samples of `v` (mfm_samples.hpp): w_new[S][U], V_new[S][U][K].
void run_foldin(mfm_foldin *p, const SampleView &v, const double *alpha, const double *mu, const double *lam, int draw, uint64_t seed,
                double *w_new, double *V_new) {
  const int S = v.count(), K = v.K;
  if (v.device != p->device) throw Error(MFM_ERR_INVALID, "fold-in observations and sample store live on different devices");
  if (v.D != p->D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  if (K > FOLDIN_MAX_RANK)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(FOLDIN_MAX_RANK) + ", the samples have rank " + std::to_string(K));
  if (S > 65535) throw Error(MFM_ERR_INVALID, "at most 65535 samples per call");
  if (!alpha || !mu || !lam) throw Error(MFM_ERR_INVALID, "no hyper-parameter arrays");
  if (!w_new || (K > 0 && !V_new)) throw Error(MFM_ERR_INVALID, "no output array");
  const int off = p->lin ? 1 : 0, M = K + off;
  for (int s = 0; s < S; s++) {
    if (!(alpha[s] > 0.0) || !std::isfinite(alpha[s]))
      throw Error(MFM_ERR_INVALID, "fold-in: the noise precision of sample " + std::to_string(s) + " is not positive and finite");
    for (int j = 1 - off; j < K + 1; j++) {
      const double l = lam[(size_t)s * (K + 1) + j], m = mu[(size_t)s * (K + 1) + j];
      if (!(l > 0.0) || !std::isfinite(l) || !std::isfinite(m))
        throw Error(MFM_ERR_INVALID, "fold-in: sample " + std::to_string(s) + " has a prior precision that is not positive and finite, or a "
                                         "prior mean that is not finite (component " + std::to_string(j) + ")");
    }
  }
  const int64_t U = p->U;
  if (U == 0) return;
  if (M == 0) {  // rank 0 without a linear term: nothing to estimate
    std::fill(w_new, w_new + (size_t)S * U, 0.0);
    return;
  }
  hipStream_t st = p->stream;
  // a store's device-to-device copies (training stream) must be complete: this stream waits for the latest one's event
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(st, v.pushed, 0));

  DevBuf<const double *> d_wv;
  DevBuf<double> d_w0, d_alpha, d_mu, d_lam;
  DevBuf<int> d_err;
  d_wv.upload(v.wv);
  d_w0.upload(v.w0);
  d_alpha.upload(alpha, (size_t)S);
  d_mu.upload(mu, (size_t)S * (K + 1));
  d_lam.upload(lam, (size_t)S * (K + 1));
  d_err.alloc_zero(1, st);

  // ---- the chunks: whole sample ranges of as many entities as the bound holds; below one entity's worth, ranges of samples
  const int64_t cells = std::max<int64_t>(p->scratch_bound / ((int64_t)(K + 1) * (int64_t)sizeof(double)), 1);
  const int Sc = (int)std::min<int64_t>(S, cells);
  const int64_t Uc = std::min<int64_t>({U, std::max<int64_t>(cells / Sc, 1), (int64_t)2147483647});
  DevBuf<double> ow, oV;
  ow.alloc((size_t)Sc * Uc);
  oV.alloc(std::max<size_t>((size_t)Sc * Uc * K, 1));

  FoldinArgs a;
  a.rowptr = p->ptr.p;
  a.colidx = p->idx.p;
  a.val = p->val.p;
  a.y = p->y.p;
  a.eoff = p->eoff.p;
  a.wv = (const double *const *)d_wv.p;
  a.w0 = d_w0.p;
  a.alpha = d_alpha.p;
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
  const size_t lds = foldin_lds_bytes(M);
  for (int64_t u0 = 0; u0 < U; u0 += Uc) {
    const int64_t nu = std::min(Uc, U - u0);
    for (int s0 = 0; s0 < S; s0 += Sc) {
      const int ns = std::min(Sc, S - s0);
      a.u0 = u0;
      a.s0 = s0;
      const dim3 grid((unsigned)nu, (unsigned)ns);
      if (draw)
        launch_foldin<true>(st, grid, lds, a);
      else
        launch_foldin<false>(st, grid, lds, a);
      MFM_HIP_CHECK(hipGetLastError());
      // the chunk's rows [ns][nu] into w_new[S][U] at (s0, u0), [ns][nu * K] into V_new[S][U * K] at (s0, u0 * K)
      MFM_HIP_CHECK(hipMemcpy2DAsync(w_new + (size_t)s0 * U + u0, (size_t)U * sizeof(double), ow.p, (size_t)nu * sizeof(double),
                                     (size_t)nu * sizeof(double), (size_t)ns, hipMemcpyDeviceToHost, st));
      if (K > 0)
        MFM_HIP_CHECK(hipMemcpy2DAsync(V_new + ((size_t)s0 * U + u0) * K, (size_t)U * K * sizeof(double), oV.p,
                                       (size_t)nu * K * sizeof(double), (size_t)nu * K * sizeof(double), (size_t)ns,
                                       hipMemcpyDeviceToHost, st));
      MFM_HIP_CHECK(hipStreamSynchronize(st));
    }
  }
  int h_err = 0;
  MFM_HIP_CHECK(hipMemcpyAsync(&h_err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  MFM_HIP_CHECK(hipStreamSynchronize(st));
  if (h_err)
    throw Error(MFM_ERR_INVALID, "fold-in: a posterior precision matrix is not positive definite (a non-finite or non-positive prior "
                                 "precision, noise precision or model value); no result is returned");
}

}  // namespace

extern "C" {

int mfm_foldin_create(int device, int64_t D, int64_t n, const int64_t *indptr, const int32_t *indices, const double *data,
                      const double *y, int64_t U, const int64_t *entity_offsets, int32_t fit_linear, mfm_foldin **out) {
  *out = nullptr;
  try {
    // (the arguments first: a machine without a GPU still learns that they are wrong)
    if (D < 0 || n < 0 || U < 0) throw Error(MFM_ERR_INVALID, "fold-in: negative shape");
    if (!indptr || !entity_offsets || (n > 0 && !y)) throw Error(MFM_ERR_INVALID, "fold-in: no index arrays");
    if (indptr[0] != 0) throw Error(MFM_ERR_INVALID, "fold-in X: indptr[0] must be 0");
    for (int64_t i = 0; i < n; i++)
      if (indptr[i + 1] < indptr[i]) throw Error(MFM_ERR_INVALID, "fold-in X: indptr must be non-decreasing");
    for (int64_t q = 0; q < indptr[n]; q++)
      if (indices[q] < 0 || indices[q] >= D) throw Error(MFM_ERR_INVALID, "fold-in X: column index out of range");
    if (entity_offsets[0] != 0 || entity_offsets[U] != n)
      throw Error(MFM_ERR_INVALID, "fold-in: the entity offsets must run from 0 to the number of observations");
    for (int64_t u = 0; u < U; u++)
      if (entity_offsets[u + 1] < entity_offsets[u]) throw Error(MFM_ERR_INVALID, "fold-in: the entity offsets must be non-decreasing");
    for (int64_t i = 0; i < n; i++)
      if (!std::isfinite(y[i])) throw Error(MFM_ERR_INVALID, "fold-in: y holds a value that is not finite");
    for (int64_t q = 0; q < indptr[n]; q++)
      if (!std::isfinite(data[q])) throw Error(MFM_ERR_INVALID, "fold-in X holds a value that is not finite");
    const int nd = mfm_device_count();
    if (nd <= 0)
      throw Error(MFM_ERR_DEVICE, "no HIP device is visible: libmyfm_hip.so has no CPU fallback (fold-in runs on MI355X only)");
    if (device < 0 || device >= nd) throw Error(MFM_ERR_INVALID, "device index out of range");
    std::unique_ptr<mfm_foldin> p(new mfm_foldin());
    p->device = device;
    p->use_device();
    MFM_HIP_CHECK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->D = D;
    p->n = n;
    p->U = U;
    p->lin = fit_linear != 0;
    p->ptr.upload(indptr, (size_t)n + 1);
    p->idx.upload(indices, (size_t)indptr[n]);
    p->val.upload(data, (size_t)indptr[n]);
    p->y.upload(y, (size_t)n);
    p->eoff.upload(entity_offsets, (size_t)U + 1);
    p->h_eoff.assign(entity_offsets, entity_offsets + U + 1);
    p->h_y.assign(y, y + n);
    *out = p.release();
    return MFM_OK;
  } catch (const mfm::Error &ex) {
    g_foldin_error = ex.what();
    return ex.code;
  } catch (const std::exception &ex) {
    g_foldin_error = ex.what();
    return MFM_ERR_RUNTIME;
  }
}

void mfm_foldin_destroy(mfm_foldin *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  delete p;
}

const char *mfm_foldin_last_error(const mfm_foldin *p) { return p ? p->err.c_str() : g_foldin_error.c_str(); }

int mfm_foldin_set_scratch_bound(mfm_foldin *p, int64_t bytes) {
  FOLDIN_TRY(p)
  if (bytes < 1) throw Error(MFM_ERR_INVALID, "the scratch bound must be positive");
  p->scratch_bound = bytes;
  FOLDIN_CATCH(p)
}

int mfm_foldin_max_rank(void) { return FOLDIN_MAX_RANK; }

int mfm_foldin_solve_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, const double *alpha, const double *mu,
                           const double *lambda, int32_t draw, uint64_t seed, double *w_new, double *V_new) {
  FOLDIN_TRY(p)
  if (!st) throw Error(MFM_ERR_INVALID, "no sample store");
  run_foldin(p, samples_of_store(st, first, count), alpha, mu, lambda, draw, seed, w_new, V_new);
  FOLDIN_CATCH(p)
}

int mfm_foldin_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     const double *alpha, const double *mu, const double *lambda, int32_t draw, uint64_t seed, double *w_new,
                     double *V_new) {
  FOLDIN_TRY(p)
  if (rank > FOLDIN_MAX_RANK)  // (before the samples are uploaded)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(FOLDIN_MAX_RANK) + ", the samples have rank " + std::to_string(rank));
  run_foldin(p, samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs), alpha, mu, lambda, draw, seed, w_new, V_new);
  FOLDIN_CATCH(p)
}

}  // extern "C"
