// mfm_foldin_handle.hpp -- the handle of mfm_foldin_* (include/myfm_hip.h): the observations of the new entities, resident on the
// device for the handle's life. Shared by mfm_foldin.hip (create, destroy, the closed-form solve) and mfm_foldin_gibbs.hip (the
// inner chain of the probit tasks).
#pragma once
#include "mfm_common.hpp"

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
