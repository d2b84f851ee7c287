// mfm_foldin_rank.hip -- mfm_foldin_rank_*: the candidates of a new entity scored and ranked under the entity's own posterior (kernels
// and algebra: mfm_foldin_rank.hpp), on the handle of mfm_foldin_create.
//
// Memory rule. The candidate table -- z of every (sample, candidate) in fragment order and f, S * Ipad * (4 KS4 + 1) doubles -- is
// built once per call and stays resident (the rule of the pair scorer's candidate side): a table above
// MFM_STORE_MAX_FRACTION of the free device memory is refused before anything is launched. The kept operands cost
// S * RT * KS4 * 64 doubles per entity (14 KB per (entity, sample) at rank 32): the entities are walked in chunks whose operands and
// outputs stay under the handle's scratch bound (mfm_foldin_set_scratch_bound), whole blocks of FRANK_EB entities and never less
// than one. A result does not depend on the chunking.
#include "mfm_foldin_rank.hpp"
#include "mfm_foldin_handle.hpp"
#include "mfm_samples.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

using namespace mfm;

namespace {

struct RankRequest {
  bool dense = false;
  int by = 0, k = 0;  // by: 0 the upper confidence bound mean + beta std, 1 the information gain
  double beta = 0.0;
  double *mean = nullptr, *sd = nullptr, *sd_within = nullptr, *gain = nullptr;  // dense: (U, I); lists: (U, k) (no sd_within)
  int64_t *idx = nullptr;
  double *value = nullptr;
};

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

// stripes of a candidate walk of `steps_total` steps for `n_tiles` row blocks: enough workgroups to fill the device twice, at most
// PAIRS_MAX_STRIPES lists to merge, no empty stripe (the pair scorer's rule)
void split_stripes(int64_t n_tiles, int64_t steps_total, int64_t &n_stripes, int64_t &steps) {
  const int64_t n = std::max<int64_t>(1, std::min<int64_t>({(512 + n_tiles - 1) / n_tiles, steps_total, (int64_t)PAIRS_MAX_STRIPES}));
  steps = (steps_total + n - 1) / n;
  n_stripes = (steps_total + steps - 1) / steps;
}

// the checks of a call that need neither samples nor a device
void check_request(const mfm_foldin *p, const RankRequest &rq) {
  if (p->I < 0) throw Error(MFM_ERR_INVALID, "fold-in ranking: no candidates set (mfm_foldin_rank_set_candidates)");
  if (rq.dense) {
    if (!rq.mean || !rq.sd || !rq.sd_within || !rq.gain) throw Error(MFM_ERR_INVALID, "no output array");
    if ((double)p->U * (double)p->I > 16777216.0)
      throw Error(MFM_ERR_INVALID, "fold-in ranking: the dense form writes at most 2^24 pairs per call (entities * candidates)");
    return;
  }
  if (rq.by != 0 && rq.by != 1) throw Error(MFM_ERR_INVALID, "fold-in ranking: by must be 0 (ucb) or 1 (gain)");
  if (rq.k < 1 || rq.k > PAIRS_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  if (!std::isfinite(rq.beta)) throw Error(MFM_ERR_INVALID, "beta must be finite");
  if (!rq.idx || !rq.value || !rq.mean || !rq.sd || !rq.gain) throw Error(MFM_ERR_INVALID, "no output array");
}

void run_rank(mfm_foldin *p, const SampleView &v, const double *alpha, const double *mu, const double *lam, const RankRequest &rq) {
  const int S = v.count(), K = v.K;
  foldin_check_samples(p, v);
  foldin_check_hyper_arrays(alpha, mu, lam);
  const int off = p->lin ? 1 : 0, M = K + off;
  foldin_check_hypers(S, K, off, alpha, mu, lam);
  const int64_t U = p->U, I = p->I;
  const int k = rq.k;
  if (U == 0) return;
  if (I == 0 || S == 0) {  // nothing to rank: empty lists
    if (!rq.dense)
      for (int64_t e = 0; e < U * k; e++) {
        rq.idx[e] = -1;
        rq.value[e] = -std::numeric_limits<double>::infinity();
        rq.mean[e] = rq.sd[e] = rq.gain[e] = std::numeric_limits<double>::quiet_NaN();
      }
    return;
  }
  hipStream_t st = p->stream;
  const int KS4 = foldin_keep_ksteps(M), RT = foldin_keep_tiles(M);
  const int64_t Ipad = round_up(I, FRANK_STEP), W = (I + 31) / 32;
  const size_t opnd = foldin_keep_doubles(M), stage = frank_stage_doubles(KS4);
  int lds_max = 0;
  MFM_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, p->device));
  if (stage * sizeof(double) > (size_t)lds_max)
    throw Error(MFM_ERR_RUNTIME, "fold-in ranking: a stage of candidates (" + std::to_string(stage * sizeof(double)) +
                                     " bytes) exceeds the device's local memory per workgroup");
  const int nbuf = 2 * stage * sizeof(double) <= (size_t)lds_max ? 2 : 1;
  {
    const double table = (double)S * (double)Ipad * (4.0 * KS4 + 1.0) * 8.0;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && table > env_double("MFM_STORE_MAX_FRACTION", 0.5) * (double)free_b)
      throw Error(MFM_ERR_RUNTIME, "fold-in ranking: the candidate table (" + std::to_string((int64_t)(table / 1048576.0)) +
                                       " MB for all samples) exceeds MFM_STORE_MAX_FRACTION of the free device memory; rank fewer "
                                       "candidates or fewer samples per call");
  }

  const FoldinStaged staged(p, v, alpha, mu, lam);

  // ---- the candidate table
  DevBuf<double> Zf, F;
  Zf.alloc(std::max<size_t>((size_t)S * (Ipad >> 4) * KS4 * 64, 1));
  F.alloc((size_t)S * Ipad);
  hipLaunchKernelGGL(k_foldin_rank_cand, dim3((unsigned)(Ipad / FOLDIN_ROWS), (unsigned)S), dim3(FOLDIN_WG),
                     foldin_rows_lds_doubles(M) * sizeof(double), st, staged.args(0, true), I, Ipad, Zf.p, F.p);
  MFM_HIP_CHECK(hipGetLastError());

  // ---- the entity chunks
  const int64_t steps_total = (I + FRANK_STEP - 1) / FRANK_STEP, sel_steps_total = (I + 63) / 64;
  const double per_entity = (double)S * ((double)opnd + K + 1) * 8.0 +
                            (rq.dense ? 4.0 * (double)I * 8.0 : (double)I * 8.0 + (double)W * 4.0 + (double)(PAIRS_MAX_STRIPES + 1) * k * 12.0 + k * 28.0);
  int64_t Uc = (int64_t)std::min<double>((double)p->scratch_bound / per_entity, 1e12);
  Uc = std::max<int64_t>(Uc / FRANK_EB * FRANK_EB, FRANK_EB);
  Uc = std::min<int64_t>(Uc, round_up(U, FRANK_EB));

  DevBuf<double> Wf, ow, oV, d_out[4], list_v, out_v, out_m, out_s, out_g;
  DevBuf<int32_t> list_i, out_i;
  DevBuf<uint32_t> mask;
  std::vector<int32_t> h_idx;
  Wf.alloc(std::max<size_t>((size_t)Uc * S * opnd, 1));
  ow.alloc((size_t)Uc * S);
  oV.alloc(std::max<size_t>((size_t)Uc * S * K, 1));
  for (int j = 0; j < (rq.dense ? 4 : 1); j++) d_out[j].alloc((size_t)Uc * I);

  FoldinArgs fa = staged.args(0);
  fa.out_w = ow.p;
  fa.out_V = oV.p;
  fa.Wf = Wf.p;
  fa.S_all = S;

  FoldinRankArgs ra;
  ra.Wf = Wf.p;
  ra.Zf = Zf.p;
  ra.F = F.p;
  ra.alpha = staged.alpha.p;
  ra.M = M;
  ra.KS4 = KS4;
  ra.RT = RT;
  ra.S = S;
  ra.nbuf = nbuf;
  ra.I = I;
  ra.Ipad = Ipad;
  ra.beta = rq.beta;
  ra.by_gain = rq.by;
  ra.mean = d_out[0].p;
  ra.sd = d_out[1].p;
  ra.sd_within = d_out[2].p;
  ra.gain = d_out[3].p;
  ra.value = d_out[0].p;
  const size_t tile_lds = (size_t)nbuf * stage * sizeof(double);
  static DeviceOnce raised_keep, raised_dense, raised_value, raised_select;
  foldin_raise_lds(k_foldin<false, true>, raised_keep, (int)foldin_lds_bytes(FOLDIN_MAX_RANK + 1));
  if (rq.dense)
    foldin_raise_lds(k_foldin_rank_tile<true>, raised_dense, lds_max);
  else {
    foldin_raise_lds(k_foldin_rank_tile<false>, raised_value, lds_max);
    foldin_raise_lds(k_foldin_rank_select, raised_select, (int)PairsSel<1>::BYTES);
  }

  for (int64_t u0 = 0; u0 < U; u0 += Uc) {
    const int64_t nu = std::min(Uc, U - u0);
    if (M > 0) {  // (rank 0 without a linear term: nothing to estimate, v = 0 and m = f)
      fa.u0 = u0;
      hipLaunchKernelGGL((k_foldin<false, true>), dim3((unsigned)nu, (unsigned)S), dim3(FOLDIN_WG), foldin_lds_bytes(M), st, fa);
      MFM_HIP_CHECK(hipGetLastError());
    }
    const int64_t n_blocks = (nu + FRANK_EB - 1) / FRANK_EB;
    int64_t n_stripes, steps;
    split_stripes(n_blocks, steps_total, n_stripes, steps);
    ra.Uc = nu;
    ra.stripe_len = steps * FRANK_STEP;
    const dim3 grid((unsigned)n_blocks, (unsigned)n_stripes);
    if (rq.dense) {
      hipLaunchKernelGGL(k_foldin_rank_tile<true>, grid, dim3(FOLDIN_WG), tile_lds, st, ra);
      MFM_HIP_CHECK(hipGetLastError());
      double *host[4] = {rq.mean, rq.sd, rq.sd_within, rq.gain};
      for (int j = 0; j < 4; j++)
        MFM_HIP_CHECK(hipMemcpyAsync(host[j] + (size_t)u0 * I, d_out[j].p, (size_t)(nu * I) * sizeof(double), hipMemcpyDeviceToHost, st));
      MFM_HIP_CHECK(hipStreamSynchronize(st));
      continue;
    }
    hipLaunchKernelGGL(k_foldin_rank_tile<false>, grid, dim3(FOLDIN_WG), tile_lds, st, ra);
    MFM_HIP_CHECK(hipGetLastError());
    // ---- the selection: exclusion mask, the stripes' lists, the merge (mfm_pairs.hpp), then the listed entries' moments
    const int64_t list_rows = round_up(nu, 16), n_tiles = list_rows / 16;
    int64_t sel_stripes, sel_steps;
    split_stripes(n_tiles, sel_steps_total, sel_stripes, sel_steps);
    PairsArgs pa;
    pa.dense = d_out[0].p;
    pa.Uc = nu;
    pa.I = I;
    pa.stripe_len = sel_steps * 64;
    pa.W = W;
    pa.k = k;
    pa.list_rows = list_rows;
    if (p->has_exclude && p->h_eptr[u0 + nu] > p->h_eptr[u0]) {
      if (mask.n < (size_t)(nu * W)) mask.alloc((size_t)(Uc * W));
      MFM_HIP_CHECK(hipMemsetAsync(mask.p, 0, (size_t)(nu * W) * sizeof(uint32_t), st));
      hipLaunchKernelGGL(k_pairs_mask, dim3((unsigned)((nu + 3) / 4)), dim3(PAIRS_WG), 0, st, p->e_ptr.p, p->e_idx.p, u0, nu, W, mask.p);
      pa.mask = mask.p;
    }
    if (list_v.n < (size_t)(sel_stripes * list_rows * k)) {
      list_v.alloc((size_t)(PAIRS_MAX_STRIPES * round_up(Uc, 16) * k));
      list_i.alloc((size_t)(PAIRS_MAX_STRIPES * round_up(Uc, 16) * k));
      out_v.alloc((size_t)(Uc * k));
      out_i.alloc((size_t)(Uc * k));
      out_m.alloc((size_t)(Uc * k));
      out_s.alloc((size_t)(Uc * k));
      out_g.alloc((size_t)(Uc * k));
    }
    pa.list_v = list_v.p;
    pa.list_i = list_i.p;
    hipLaunchKernelGGL(k_foldin_rank_select, dim3((unsigned)n_tiles, (unsigned)sel_stripes), dim3(PAIRS_WG), PairsSel<1>::BYTES, st, pa);
    MFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)nu), dim3(PAIRS_WG), 0, st, list_v.p, list_i.p, (int)sel_stripes, list_rows, k, out_v.p,
                       out_i.p);
    hipLaunchKernelGGL(k_foldin_rank_at, dim3((unsigned)((nu * k + 3) / 4)), dim3(FOLDIN_WG), 0, st, ra, out_i.p, k, nu * k, out_m.p, out_s.p,
                       out_g.p);
    MFM_HIP_CHECK(hipGetLastError());
    const size_t n_e = (size_t)(nu * k), o = (size_t)(u0 * k);
    h_idx.resize(n_e);
    MFM_HIP_CHECK(hipMemcpyAsync(rq.value + o, out_v.p, n_e * sizeof(double), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipMemcpyAsync(rq.mean + o, out_m.p, n_e * sizeof(double), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipMemcpyAsync(rq.sd + o, out_s.p, n_e * sizeof(double), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipMemcpyAsync(rq.gain + o, out_g.p, n_e * sizeof(double), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), out_i.p, n_e * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    MFM_HIP_CHECK(hipStreamSynchronize(st));
    for (size_t e = 0; e < n_e; e++) rq.idx[o + e] = h_idx[e];
  }
  staged.finish("fold-in ranking: a posterior precision matrix is not positive definite (a non-finite or non-positive prior precision, "
                "noise precision or model value); no result is returned");
}

// An entry point: the request's checks, which need neither samples nor a device, then the samples, then the call
template <class From>
int rank_call(mfm_foldin *p, const From &from, const double *alpha, const double *mu, const double *lam, const RankRequest &rq) {
  return foldin_call(p, from, [&](auto samples) {
    check_request(p, rq);
    run_rank(p, samples(), alpha, mu, lam, rq);
  });
}

RankRequest dense_request(double *mean, double *sd, double *sd_within, double *gain) {
  RankRequest rq;
  rq.dense = true;
  rq.mean = mean;
  rq.sd = sd;
  rq.sd_within = sd_within;
  rq.gain = gain;
  return rq;
}

RankRequest topk_request(int by, int k, double beta, int64_t *idx, double *value, double *mean, double *sd, double *gain) {
  RankRequest rq;
  rq.by = by;
  rq.k = k;
  rq.beta = beta;
  rq.idx = idx;
  rq.value = value;
  rq.mean = mean;
  rq.sd = sd;
  rq.gain = gain;
  return rq;
}

}  // namespace

extern "C" {

int mfm_foldin_rank_set_candidates(mfm_foldin *p, int64_t I, const int64_t *indptr, const int32_t *indices, const double *data) {
  FOLDIN_TRY(p)
  if (I < 0 || I > 2147483647) throw Error(MFM_ERR_INVALID, "fold-in candidates: the row count must lie in [0, 2^31)");
  check_pattern(I, p->D, indptr, indices, "fold-in candidates");
  for (int64_t q = 0; q < indptr[I]; q++)
    if (!data || !std::isfinite(data[q])) throw Error(MFM_ERR_INVALID, "fold-in candidates hold a value that is not finite");
  p->c_ptr.upload(indptr, (size_t)I + 1);
  p->c_idx.upload(indices, (size_t)indptr[I]);
  p->c_val.upload(data, (size_t)indptr[I]);
  p->I = I;
  p->has_exclude = false;  // (a pattern belongs to one candidate set)
  FOLDIN_CATCH(p)
}

int mfm_foldin_rank_set_exclude(mfm_foldin *p, const int64_t *indptr, const int32_t *indices) {
  FOLDIN_TRY(p)
  if (p->I < 0) throw Error(MFM_ERR_INVALID, "fold-in ranking: set the candidates before the exclusion pattern");
  check_pattern(p->U, p->I, indptr, indices, "fold-in exclude");
  p->e_ptr.upload(indptr, (size_t)p->U + 1);
  p->e_idx.upload(indices, (size_t)indptr[p->U]);
  p->h_eptr.assign(indptr, indptr + p->U + 1);
  p->has_exclude = true;
  FOLDIN_CATCH(p)
}

int mfm_foldin_rank_dist_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, const double *alpha, const double *mu,
                               const double *lambda, double *mean, double *sd, double *sd_within, double *gain) {
  return rank_call(p, FoldinFromStore{st, first, count}, alpha, mu, lambda, dense_request(mean, sd, sd_within, gain));
}

int mfm_foldin_rank_dist(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                         const double *alpha, const double *mu, const double *lambda, double *mean, double *sd, double *sd_within,
                         double *gain) {
  return rank_call(p, FoldinFromHost{rank, n_samples, w0s, ws, Vs}, alpha, mu, lambda, dense_request(mean, sd, sd_within, gain));
}

int mfm_foldin_rank_topk_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, const double *alpha, const double *mu,
                               const double *lambda, int32_t by, int32_t k, double beta, int64_t *idx, double *value, double *mean,
                               double *sd, double *gain) {
  return rank_call(p, FoldinFromStore{st, first, count}, alpha, mu, lambda, topk_request(by, k, beta, idx, value, mean, sd, gain));
}

int mfm_foldin_rank_topk(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                         const double *alpha, const double *mu, const double *lambda, int32_t by, int32_t k, double beta, int64_t *idx,
                         double *value, double *mean, double *sd, double *gain) {
  return rank_call(p, FoldinFromHost{rank, n_samples, w0s, ws, Vs}, alpha, mu, lambda, topk_request(by, k, beta, idx, value, mean, sd, gain));
}

}  // extern "C"
