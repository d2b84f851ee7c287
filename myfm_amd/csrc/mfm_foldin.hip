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
#include "mfm_foldin_gibbs_plan.hpp"
#include "mfm_foldin_handle.hpp"

#include <cmath>
#include <memory>

using namespace mfm;

static thread_local std::string g_foldin_error;

namespace {

template <bool DRAW>
void launch_foldin(hipStream_t s, dim3 grid, const FoldinArgs &a) {
  static DeviceOnce raised;  // (the largest form once: rank 64 asks for 77 KB)
  foldin_raise_lds(k_foldin<DRAW>, raised, (int)foldin_lds_bytes(FOLDIN_MAX_RANK + 1));
  hipLaunchKernelGGL((k_foldin<DRAW>), grid, dim3(FOLDIN_WG), foldin_lds_bytes(a.K + a.lin), s, a);
}

// The whole call over the samples of `v` (mfm_samples.hpp): w_new[S][U], V_new[S][U][K].
void run_foldin(mfm_foldin *p, const SampleView &v, const double *alpha, const double *mu, const double *lam, int draw, uint64_t seed,
                double *w_new, double *V_new) {
  const int S = v.count(), K = v.K;
  foldin_check_samples(p, v);
  foldin_check_hyper_arrays(alpha, mu, lam);
  if (!w_new || (K > 0 && !V_new)) throw Error(MFM_ERR_INVALID, "no output array");
  const int off = p->lin ? 1 : 0, M = K + off;
  foldin_check_hypers(S, K, off, alpha, mu, lam);
  const int64_t U = p->U;
  if (U == 0) return;
  if (M == 0) {  // rank 0 without a linear term: nothing to estimate
    std::fill(w_new, w_new + (size_t)S * U, 0.0);
    return;
  }
  const FoldinStaged staged(p, v, alpha, mu, lam);
  FoldinArgs a = staged.args(seed);
  foldin_walk(p, foldin_chunks(U, S, K, p->scratch_bound), a, [&](const FoldinChunk &, dim3 grid) {
    if (draw)
      launch_foldin<true>(p->stream, grid, a);
    else
      launch_foldin<false>(p->stream, grid, a);
  }, w_new, V_new);
  staged.finish("fold-in: a posterior precision matrix is not positive definite (a non-finite or non-positive prior precision, noise "
                "precision or model value); no result is returned");
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
    check_pattern(n, D, indptr, indices, "fold-in X");
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
  return foldin_call(p, FoldinFromStore{st, first, count},
                     [&](auto samples) { run_foldin(p, samples(), alpha, mu, lambda, draw, seed, w_new, V_new); });
}

int mfm_foldin_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     const double *alpha, const double *mu, const double *lambda, int32_t draw, uint64_t seed, double *w_new,
                     double *V_new) {
  return foldin_call(p, FoldinFromHost{rank, n_samples, w0s, ws, Vs},
                     [&](auto samples) { run_foldin(p, samples(), alpha, mu, lambda, draw, seed, w_new, V_new); });
}

}  // extern "C"
