// mfm_foldin_handle.hpp -- the handle of mfm_foldin_* (include/myfm_hip.h): the observations of the new entities, resident on the
// device for the handle's life. Shared by mfm_foldin.hip (create, destroy, the closed-form solve) and mfm_foldin_gibbs.hip (the
// inner chain of the probit tasks) and mfm_foldin_rank.hip (ranking under the new entities' own posterior: the candidate
// contexts and the exclusion pattern are resident too, once set).
#pragma once
#include "mfm_common.hpp"

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

// What every closed-form call checks of its samples and hyper-parameters before anything is launched, in two steps so that a
// caller's own argument checks go between them: the samples against the handle, then alpha[S], mu / lam[S][K + 1] value by value.
inline void foldin_check_samples(const mfm_foldin *p, int device, int64_t D, int K, int S, int max_rank, const double *alpha,
                                 const double *mu, const double *lam) {
  using mfm::Error;
  if (device != p->device) throw Error(MFM_ERR_INVALID, "fold-in observations and sample store live on different devices");
  if (D != p->D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  if (K > max_rank)
    throw Error(MFM_ERR_INVALID, "fold-in serves ranks up to " + std::to_string(max_rank) + ", the samples have rank " + std::to_string(K));
  if (S > 65535) throw Error(MFM_ERR_INVALID, "at most 65535 samples per call");
  if (!alpha || !mu || !lam) throw Error(MFM_ERR_INVALID, "no hyper-parameter arrays");
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
