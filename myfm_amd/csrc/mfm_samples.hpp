// mfm_samples.hpp -- the kept posterior samples as every device predictor reads them (mfm_design_predict_store, mfm_design_summary*,
// mfm_pairs_*): a range of a device store read in place, or host samples uploaded for the call. Included by mfm_hip.hip
// (through mfm_predict.hpp, which defines the two makers next to mfm_store) and by mfm_pairs.hip.
#pragma once
#include "mfm_common.hpp"

struct mfm_store;

namespace mfm {

struct SampleView {
  int device = 0;
  int64_t D = 0;
  int K = 0;
  std::vector<const double *> wv;  // per sample, on the device: w[D] then V[K][D] (factor-major, the store's layout)
  std::vector<double> w0;
  hipEvent_t pushed = nullptr;  // behind the store's latest device-to-device snapshot: the reading stream waits for it (null: none)
  DevBuf<double> own;           // host samples: the call's upload, freed with the view
  int count() const { return (int)wv.size(); }
};

// the samples [first, first + count) of a device store
SampleView samples_of_store(mfm_store *st, int first, int count);
// n host samples (w0s[n], ws[n][D], Vs[n][rank][D]): one allocation, copied sample by sample
SampleView samples_of_host(int device, int64_t D, int rank, int n, const double *w0s, const double *ws, const double *Vs);

}  // namespace mfm
