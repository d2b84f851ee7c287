// mfm_align.hip -- mfm_align_*: one embedding per feature with an error bar out of the kept samples, by orthogonal Procrustes
// alignment of their factor matrices (kernels and algebra: mfm_align.hpp).
//
// Memory rule. Resident for the call: the result (mean and std, 2 K D doubles), the rotations (S K^2), the weights (D) and the
// partial cross products of k_align_gram, S_g chunks K^2 doubles for a group of S_g samples. The samples are walked in groups whose
// partials stay under `scratch_bound` bytes (256 MB unless mfm_align_set_scratch_bound says otherwise; never less than one sample).
// The chunk count depends on D alone and a sample's sums never cross a group, so a result does not depend on the grouping.
#include "mfm_align.hpp"
#include "mfm_samples.hpp"

#include <cmath>
#include <memory>

using namespace mfm;

struct mfm_aligner {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t D = 0;
  int64_t scratch_bound = (int64_t)256 << 20;
  ~mfm_aligner() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  void use_device() { MFM_HIP_CHECK(hipSetDevice(device)); }
};

static thread_local std::string g_align_error;

#define ALIGN_TRY(p) \
  try {              \
    (p)->use_device();
#define ALIGN_CATCH(p)               \
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

namespace {

template <class KERNEL>
void raise_lds(KERNEL k, size_t bytes, DeviceOnce &raised) {
  if (!raised.need()) return;
  MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  raised.mark();
}

template <int NT>
void launch_gram(hipStream_t s, dim3 grid, const AlignGramArgs &a) {
  static DeviceOnce raised;
  raise_lds(k_align_gram<NT>, align_gram_lds(NT), raised);
  hipLaunchKernelGGL((k_align_gram<NT>), grid, dim3(ALIGN_WG), align_gram_lds(NT), s, a);
}
template <int NT>
void launch_apply(hipStream_t s, dim3 grid, const AlignApplyArgs &a) {
  static DeviceOnce raised;
  raise_lds(k_align_apply<NT>, align_apply_lds(NT), raised);
  hipLaunchKernelGGL((k_align_apply<NT>), grid, dim3(ALIGN_WG), align_apply_lds(NT), s, a);
}
void launch_polar(hipStream_t s, dim3 grid, const AlignPolarArgs &a) {
  static DeviceOnce raised;
  raise_lds(k_align_polar, align_polar_lds(), raised);
  hipLaunchKernelGGL(k_align_polar, grid, dim3(ALIGN_WG), align_polar_lds(), s, a);
}

void check_rank(int K) {
  if (K < 0) throw Error(MFM_ERR_INVALID, "align: negative rank");
  if (K > ALIGN_MAX_RANK)
    throw Error(MFM_ERR_INVALID, "align serves ranks up to " + std::to_string(ALIGN_MAX_RANK) + ", the samples have rank " + std::to_string(K));
}

// The whole call over the samples of `v` (mfm_samples.hpp). mean, std [K][D] factor-major, rotations [S][K][K], alignment [S].
void run_align(mfm_aligner *p, const SampleView &v, int reference, int n_refine, const double *weights, double *mean, double *std,
               double *rotations, double *alignment) {
  const int S = v.count(), K = v.K;
  const int64_t D = p->D;
  if (v.device != p->device) throw Error(MFM_ERR_INVALID, "align: the handle and the sample store live on different devices");
  if (v.D != D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  check_rank(K);
  if (S < 1) throw Error(MFM_ERR_INVALID, "align: no samples");
  if (S > 65535 * ALIGN_GROUP) throw Error(MFM_ERR_INVALID, "align: at most " + std::to_string(65535 * ALIGN_GROUP) + " samples per call");
  if (reference < -S || reference >= S)
    throw Error(MFM_ERR_INVALID, "align: reference " + std::to_string(reference) + " is out of range for " + std::to_string(S) + " samples");
  if (reference < 0) reference += S;
  if (n_refine < 0 || n_refine > 8) throw Error(MFM_ERR_INVALID, "align: n_refine must lie in [0, 8]");
  if (weights)
    for (int64_t d = 0; d < D; d++)
      if (!(weights[d] >= 0.0) || !std::isfinite(weights[d]))
        throw Error(MFM_ERR_INVALID, "align: weight " + std::to_string(d) + " is negative or not finite");
  if (!alignment || (K > 0 && (!rotations || (D > 0 && (!mean || !std))))) throw Error(MFM_ERR_INVALID, "align: no output array");
  std::fill(alignment, alignment + S, 0.0);
  if (K == 0) return;  // nothing to align: no launch

  hipStream_t st = p->stream;
  // a store's device-to-device copies (training stream) must be complete: this stream waits for the latest one's event
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(st, v.pushed, 0));
  std::vector<const double *> hV((size_t)S);
  for (int s = 0; s < S; s++) hV[s] = v.wv[s] + D;
  DevBuf<const double *> dV;
  DevBuf<double> dc, dmean, dstd, dR, dal, part, nv, nr;
  dV.upload(hV);
  if (weights) dc.upload(weights, (size_t)D);
  const size_t KK = (size_t)K * K;
  const int nchunks = align_chunks(D), NT = (K + 15) / 16;
  const int Sg = (int)std::min<int64_t>(S, std::max<int64_t>(p->scratch_bound / (int64_t)(std::max(nchunks, 1) * KK * sizeof(double)), 1));
  dmean.alloc(std::max<size_t>((size_t)K * D, 1));
  dstd.alloc(std::max<size_t>((size_t)K * D, 1));
  dR.alloc((size_t)S * KK);
  dal.alloc((size_t)S);
  part.alloc(std::max<size_t>((size_t)Sg * nchunks * KK, 1));
  nv.alloc(std::max<size_t>((size_t)Sg * nchunks, 1));
  nr.alloc(std::max<size_t>((size_t)nchunks, 1));

  for (int round = 0; round <= n_refine; round++) {
    for (int s0 = 0; s0 < S; s0 += Sg) {
      const int ns = std::min(Sg, S - s0);
      if (nchunks > 0) {
        AlignGramArgs g;
        g.V = dV.p;
        g.ref = round == 0 ? hV[(size_t)reference] : dmean.p;
        g.c = dc.p;
        g.D = D;
        g.K = K;
        g.s0 = s0;
        g.ns = ns;
        g.nchunks = nchunks;
        g.part = part.p;
        g.nv = nv.p;
        g.nr = nr.p;
        g.write_nr = s0 == 0;
        const dim3 grid((unsigned)nchunks, (unsigned)((ns + ALIGN_GROUP - 1) / ALIGN_GROUP));
        switch (NT) {
          case 1: launch_gram<1>(st, grid, g); break;
          case 2: launch_gram<2>(st, grid, g); break;
          case 3: launch_gram<3>(st, grid, g); break;
          default: launch_gram<4>(st, grid, g); break;
        }
        MFM_HIP_CHECK(hipGetLastError());
      }
      AlignPolarArgs q;
      q.part = part.p;
      q.nv = nv.p;
      q.nr = nr.p;
      q.K = K;
      q.nchunks = nchunks;
      q.s0 = s0;
      q.R = dR.p;
      q.align = dal.p;
      launch_polar(st, dim3((unsigned)ns), q);
      MFM_HIP_CHECK(hipGetLastError());
    }
    if (D > 0) {
      AlignApplyArgs y;
      y.V = dV.p;
      y.R = dR.p;
      y.D = D;
      y.K = K;
      y.S = S;
      y.mean = dmean.p;
      y.std = dstd.p;
      const dim3 grid((unsigned)((D + ALIGN_TILE - 1) / ALIGN_TILE));
      switch (NT) {
        case 1: launch_apply<1>(st, grid, y); break;
        case 2: launch_apply<2>(st, grid, y); break;
        case 3: launch_apply<3>(st, grid, y); break;
        default: launch_apply<4>(st, grid, y); break;
      }
      MFM_HIP_CHECK(hipGetLastError());
    }
  }
  if (D > 0) {
    MFM_HIP_CHECK(hipMemcpyAsync(mean, dmean.p, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipMemcpyAsync(std, dstd.p, (size_t)K * D * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  MFM_HIP_CHECK(hipMemcpyAsync(rotations, dR.p, (size_t)S * KK * sizeof(double), hipMemcpyDeviceToHost, st));
  MFM_HIP_CHECK(hipMemcpyAsync(alignment, dal.p, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
  MFM_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

extern "C" {

int mfm_align_create(int device, int64_t D, mfm_aligner **out) {
  *out = nullptr;
  try {
    if (D < 0) throw Error(MFM_ERR_INVALID, "align: negative feature size");
    const int nd = mfm_device_count();
    if (nd <= 0) throw Error(MFM_ERR_DEVICE, "no HIP device is visible: libmyfm_hip.so has no CPU fallback (alignment runs on MI355X only)");
    if (device < 0 || device >= nd) throw Error(MFM_ERR_INVALID, "device index out of range");
    std::unique_ptr<mfm_aligner> p(new mfm_aligner());
    p->device = device;
    p->D = D;
    p->use_device();
    MFM_HIP_CHECK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    *out = p.release();
    return MFM_OK;
  } catch (const mfm::Error &ex) {
    g_align_error = ex.what();
    return ex.code;
  } catch (const std::exception &ex) {
    g_align_error = ex.what();
    return MFM_ERR_RUNTIME;
  }
}

void mfm_align_destroy(mfm_aligner *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  delete p;
}

const char *mfm_align_last_error(const mfm_aligner *p) { return p ? p->err.c_str() : g_align_error.c_str(); }

int mfm_align_set_scratch_bound(mfm_aligner *p, int64_t bytes) {
  ALIGN_TRY(p)
  if (bytes < 1) throw Error(MFM_ERR_INVALID, "the scratch bound must be positive");
  p->scratch_bound = bytes;
  ALIGN_CATCH(p)
}

int mfm_align_max_rank(void) { return ALIGN_MAX_RANK; }

int mfm_align_store(mfm_aligner *p, mfm_store *st, int32_t first, int32_t count, int32_t reference, int32_t n_refine,
                    const double *weights, double *mean, double *std, double *rotations, double *alignment) {
  ALIGN_TRY(p)
  if (!st) throw Error(MFM_ERR_INVALID, "no sample store");
  run_align(p, samples_of_store(st, first, count), reference, n_refine, weights, mean, std, rotations, alignment);
  ALIGN_CATCH(p)
}

int mfm_align(mfm_aligner *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t reference,
              int32_t n_refine, const double *weights, double *mean, double *std, double *rotations, double *alignment) {
  ALIGN_TRY(p)
  check_rank(rank);  // (before the samples are uploaded)
  run_align(p, samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs), reference, n_refine, weights, mean, std, rotations, alignment);
  ALIGN_CATCH(p)
}

}  // extern "C"
