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

using namespace mfm;

namespace {

template <int TASK, bool DRAW>
void launch_foldin_gibbs(hipStream_t s, dim3 grid, const FoldinGibbsArgs &g) {
  static DeviceOnce raised;
  foldin_raise_lds(k_foldin_gibbs<TASK, DRAW>, raised, (int)foldin_lds_bytes(FOLDIN_MAX_RANK + 1));
  hipLaunchKernelGGL((k_foldin_gibbs<TASK, DRAW>), grid, dim3(FOLDIN_WG), foldin_lds_bytes(g.a.K + g.a.lin), s, g);
}

// The whole call over the samples of `v`: w_new[S][U], V_new[S][U][K].
void run_foldin_gibbs(mfm_foldin *p, const SampleView &v, int task, int n_class, const double *cut, const double *mu, const double *lam,
                      int n_burn, int n_inner, int draw, uint64_t seed, double *w_new, double *V_new) {
  const int S = v.count(), K = v.K;
  foldin_check_samples(p, v);
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
  const int64_t *eoff = p->h_eoff.data();
  const std::vector<FoldinChunk> chunks = foldin_gibbs_plan(eoff, U, S, M, K, p->scratch_bound);
  size_t zf_max = 1;
  for (const FoldinChunk &c : chunks) zf_max = std::max(zf_max, (size_t)c.ns * (size_t)(eoff[c.u0 + c.nu] - eoff[c.u0]) * (size_t)(M + 1));

  const FoldinStaged staged(p, v, nullptr, mu, lam);
  DevBuf<double> d_cut, zf;
  if (task == FOLDIN_TASK_ORDERED) d_cut.upload(cut, (size_t)S * (n_class - 1));
  zf.alloc(zf_max);

  FoldinGibbsArgs g;
  g.a = staged.args(seed);
  g.cut = d_cut.p;
  g.n_class = n_class;
  g.n_burn = n_burn;
  g.n_inner = n_inner;
  g.n = p->n;
  g.zf = zf.p;
  foldin_walk(p, chunks, g.a, [&](const FoldinChunk &c, dim3 grid) {
    g.rows = eoff[c.u0 + c.nu] - eoff[c.u0];
    if (task == FOLDIN_TASK_ORDERED) {
      if (draw)
        launch_foldin_gibbs<FOLDIN_TASK_ORDERED, true>(st, grid, g);
      else
        launch_foldin_gibbs<FOLDIN_TASK_ORDERED, false>(st, grid, g);
    } else {
      if (draw)
        launch_foldin_gibbs<FOLDIN_TASK_CLASSIFIER, true>(st, grid, g);
      else
        launch_foldin_gibbs<FOLDIN_TASK_CLASSIFIER, false>(st, grid, g);
    }
  }, w_new, V_new);
  staged.finish("fold-in: a posterior precision matrix is not positive definite or a row's score is not finite (a non-finite model "
                "value); no result is returned");
}

}  // namespace

extern "C" {

int mfm_foldin_gibbs_solve_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, int32_t task, int32_t n_class,
                                 const double *cutpoints, const double *mu, const double *lambda, int32_t n_burn, int32_t n_inner,
                                 int32_t draw, uint64_t seed, double *w_new, double *V_new) {
  return foldin_call(p, FoldinFromStore{st, first, count}, [&](auto samples) {
    run_foldin_gibbs(p, samples(), task, n_class, cutpoints, mu, lambda, n_burn, n_inner, draw, seed, w_new, V_new);
  });
}

int mfm_foldin_gibbs_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t task, int32_t n_class, const double *cutpoints, const double *mu, const double *lambda,
                           int32_t n_burn, int32_t n_inner, int32_t draw, uint64_t seed, double *w_new, double *V_new) {
  return foldin_call(p, FoldinFromHost{rank, n_samples, w0s, ws, Vs}, [&](auto samples) {
    run_foldin_gibbs(p, samples(), task, n_class, cutpoints, mu, lambda, n_burn, n_inner, draw, seed, w_new, V_new);
  });
}

}  // extern "C"
