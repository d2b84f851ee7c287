// mfm_foldin_handle.hpp -- the handle of mfm_foldin_* (include/myfm_hip.h): the observations of the new entities, resident on the
// device for the handle's life. Shared by mfm_foldin.hip (create, destroy, the closed-form solve) and mfm_foldin_gibbs.hip (the
// inner chain of the probit tasks) and mfm_foldin_rank.hip (ranking under the new entities' own posterior: the candidate
// contexts and the exclusion pattern are resident too, once set). Below the handle, what a call of any of the three does in the
// same way: where its samples come from (foldin_call), their checks, their staging on the device with the kernels' error word
// (FoldinStaged), the raise of a kernel's LDS limit and, for the two solvers, the walk over the chunks (foldin_walk).
#pragma once
#include "mfm_common.hpp"
#include "mfm_foldin.hpp"
#include "mfm_samples.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

struct mfm_foldin {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t D = 0, n = 0, U = 0;
  bool lin = true;
  mfm::DevBuf<int64_t> ptr, eoff;
  mfm::DevBuf<int32_t> idx;
  mfm::DevBuf<double> val, y;
  std::vector<int64_t> h_eoff;  // host copies for the chunk plan and the label checks of mfm_foldin_gibbs_*
  std::vector<double> h_y;
  int64_t scratch_bound = (int64_t)256 << 20;
  // mfm_foldin_rank_*: the candidate contexts (I, D) as CSR (I < 0: none set) and the (U, I) exclusion pattern
  int64_t I = -1;
  mfm::DevBuf<int64_t> c_ptr, e_ptr;
  mfm::DevBuf<int32_t> c_idx, e_idx;
  mfm::DevBuf<double> c_val;
  std::vector<int64_t> h_eptr;
  bool has_exclude = false;
  ~mfm_foldin() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  void use_device() { MFM_HIP_CHECK(hipSetDevice(device)); }
};

#define FOLDIN_TRY(p) \
  try {               \
    (p)->use_device();
#define FOLDIN_CATCH(p)              \
  return MFM_OK;                     \
  }                                  \
  catch (const mfm::Error &ex) {     \
    (p)->err = ex.what();            \
    return ex.code;                  \
  }                                  \
  catch (const std::exception &ex) { \
    (p)->err = ex.what();            \
    return MFM_ERR_RUNTIME;          \
  }

// a CSR pattern of `rows` rows over `cols` columns, from outside
inline void check_pattern(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, const char *what) {
  using mfm::Error;
  if (!indptr || (rows > 0 && indptr[rows] > 0 && !indices)) throw Error(MFM_ERR_INVALID, std::string(what) + ": no index arrays");
  if (indptr[0] != 0) throw Error(MFM_ERR_INVALID, std::string(what) + ": indptr[0] must be 0");
  for (int64_t i = 0; i < rows; i++)
    if (indptr[i + 1] < indptr[i]) throw Error(MFM_ERR_INVALID, std::string(what) + ": indptr must be non-decreasing");
  for (int64_t q = 0; q < indptr[rows]; q++)
    if (indices[q] < 0 || indices[q] >= cols) throw Error(MFM_ERR_INVALID, std::string(what) + ": column index out of range");
}

// ---- where a call's samples come from: all that the _store and the host twin of an entry point differ in ---------------------------
struct FoldinFromStore {
  mfm_store *st;
  int first, count;
  mfm::SampleView samples(const mfm_foldin *) const {
    if (!st) throw mfm::Error(MFM_ERR_INVALID, "no sample store");
    return mfm::samples_of_store(st, first, count);
  }
};
struct FoldinFromHost {
  int rank, n_samples;
  const double *w0s, *ws, *Vs;
  mfm::SampleView samples(const mfm_foldin *p) const {
    if (rank > mfm::FOLDIN_MAX_RANK)  // (before the samples are uploaded)
      throw mfm::Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(mfm::FOLDIN_MAX_RANK) + ", the samples have rank " +
                                            std::to_string(rank));
    return mfm::samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs);
  }
};
// An entry point over samples. `body` takes the maker of the samples and calls it once, after the checks that come before them.
template <class From, class Body>
int foldin_call(mfm_foldin *p, const From &from, Body body) {
  FOLDIN_TRY(p)
  body([&] { return from.samples(p); });
  FOLDIN_CATCH(p)
}

// ---- what every call checks of its samples and hyper-parameters before anything is launched, in steps so that a caller's own
// argument checks go between them: the samples against the handle, the arrays, then alpha[S], mu / lam[S][K + 1] value by value
inline void foldin_check_samples(const mfm_foldin *p, const mfm::SampleView &v) {
  using mfm::Error;
  if (v.device != p->device) throw Error(MFM_ERR_INVALID, "fold-in observations and sample store live on different devices");
  if (v.D != p->D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  if (v.K > mfm::FOLDIN_MAX_RANK)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(mfm::FOLDIN_MAX_RANK) + ", the samples have rank " +
                                     std::to_string(v.K));
  if (v.count() > 65535) throw Error(MFM_ERR_INVALID, "at most 65535 samples per call");
}
inline void foldin_check_hyper_arrays(const double *alpha, const double *mu, const double *lam) {
  if (!alpha || !mu || !lam) throw mfm::Error(MFM_ERR_INVALID, "no hyper-parameter arrays");
}
inline void foldin_check_hypers(int S, int K, int off, const double *alpha, const double *mu, const double *lam) {
  using mfm::Error;
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
}

// ---- the samples and hyper-parameters of a call on the device, with the error word of its kernels ---------------------------------
struct FoldinStaged {
  const mfm_foldin *p;
  int K;
  mfm::DevBuf<const double *> wv;
  mfm::DevBuf<double> w0, alpha, mu, lam;
  mfm::DevBuf<int> err;
  // alpha: null where the kernels read none (the probit chain)
  FoldinStaged(const mfm_foldin *p, const mfm::SampleView &v, const double *h_alpha, const double *h_mu, const double *h_lam) : p(p), K(v.K) {
    const size_t S = (size_t)v.count();
    // a store's device-to-device copies (training stream) must be complete: this stream waits for the latest one's event
    if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(p->stream, v.pushed, 0));
    wv.upload(v.wv);
    w0.upload(v.w0);
    if (h_alpha) alpha.upload(h_alpha, S);
    mu.upload(h_mu, S * (K + 1));
    lam.upload(h_lam, S * (K + 1));
    err.alloc_zero(1, p->stream);
  }
  // The arguments that no launch of the call changes, over the handle's observations or (candidates) its candidate contexts, which
  // have neither targets nor entities. The launch's u0, s0, the outputs and the KEEP fields are the caller's.
  mfm::FoldinArgs args(uint64_t seed, bool candidates = false) const {
    mfm::FoldinArgs a;
    a.rowptr = candidates ? p->c_ptr.p : p->ptr.p;
    a.colidx = candidates ? p->c_idx.p : p->idx.p;
    a.val = candidates ? p->c_val.p : p->val.p;
    a.y = candidates ? nullptr : p->y.p;
    a.eoff = candidates ? nullptr : p->eoff.p;
    a.wv = (const double *const *)wv.p;
    a.w0 = w0.p;
    a.alpha = alpha.p;
    a.mu = mu.p;
    a.lam = lam.p;
    a.D = p->D;
    a.U = p->U;
    a.u0 = 0;
    a.s0 = 0;
    a.K = K;
    a.lin = p->lin ? 1 : 0;
    a.seed = seed;
    a.out_w = a.out_V = nullptr;
    a.err = err.p;
    return a;
  }
  // the end of a call: `refusal` is thrown when a cell has set the error word
  void finish(const char *refusal) const {
    int h_err = 0;
    MFM_HIP_CHECK(hipMemcpyAsync(&h_err, err.p, sizeof(int), hipMemcpyDeviceToHost, p->stream));
    MFM_HIP_CHECK(hipStreamSynchronize(p->stream));
    if (h_err) throw mfm::Error(MFM_ERR_INVALID, refusal);
  }
};

// a kernel's limit of dynamic LDS, raised once per device
template <class Kern>
void foldin_raise_lds(Kern kernel, mfm::DeviceOnce &raised, int bytes) {
  if (raised.need()) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    raised.mark();
  }
}

// ---- the chunk walk of the two solvers: per chunk launch(c, grid) with a.u0 / a.s0 / a.out_w / a.out_V set (launch reads `a` where
// it captured it), then the chunk's results [ns][nu] into w_new[S][U] at (s0, u0) and [ns][nu * K] into V_new[S][U * K] at (s0, u0 * K)
// (chunks: the FoldinChunk list of mfm_foldin_gibbs_plan.hpp, which only the solvers' units include)
template <class Chunks, class Launch>
void foldin_walk(const mfm_foldin *p, const Chunks &chunks, mfm::FoldinArgs &a, Launch launch, double *w_new, double *V_new) {
  const size_t U = (size_t)p->U, K = (size_t)a.K;
  size_t cells_max = 1;
  for (const auto &c : chunks) cells_max = std::max(cells_max, (size_t)c.ns * (size_t)c.nu);
  mfm::DevBuf<double> ow, oV;
  ow.alloc(cells_max);
  oV.alloc(std::max<size_t>(cells_max * K, 1));
  a.out_w = ow.p;
  a.out_V = oV.p;
  hipStream_t st = p->stream;
  for (const auto &c : chunks) {
    a.u0 = c.u0;
    a.s0 = c.s0;
    launch(c, dim3((unsigned)c.nu, (unsigned)c.ns));
    MFM_HIP_CHECK(hipGetLastError());
    MFM_HIP_CHECK(hipMemcpy2DAsync(w_new + (size_t)c.s0 * U + c.u0, U * sizeof(double), ow.p, (size_t)c.nu * sizeof(double),
                                   (size_t)c.nu * sizeof(double), (size_t)c.ns, hipMemcpyDeviceToHost, st));
    if (K > 0)
      MFM_HIP_CHECK(hipMemcpy2DAsync(V_new + ((size_t)c.s0 * U + c.u0) * K, U * K * sizeof(double), oV.p, (size_t)c.nu * K * sizeof(double),
                                     (size_t)c.nu * K * sizeof(double), (size_t)c.ns, hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipStreamSynchronize(st));
  }
}
