// mfm_pairs.hip -- mfm_pairs_*: scores of every (query row, candidate row) pair of two sparse sides under the posterior samples, dense
// or as the per-query top-k, on the fp64 MFMA (kernels and the decomposition: mfm_pairs.hpp).
//
// Memory rule. The candidate side's embedding Q (padded candidates x samples x padded factors doubles) and its biases stay resident
// for the whole call; they are refused, before anything is allocated, when they exceed MFM_STORE_MAX_FRACTION (default 0.5) of the
// free device memory. The queries are walked in chunks of rows whose scratch -- P and the biases, the exclusion bitmask, the
// per-stripe lists at the most stripes a launch can have, the outputs -- stays under `scratch_bound` bytes (256 MB unless
// mfm_pairs_set_scratch_bound says otherwise; never less than one 64-row tile). The per-sample selecting form, whose lists scale
// with samples x row tiles, splits the bound between a chunk's own scratch and slices of its plan (walk_samples).
//
// Relation blocks (mfm_pairs_add_block). A side's row is [main | B_0[o2b_0[r]] | ...]; every block of either side gets a table
// (block rows x samples x (padded factors + 2) doubles, mfm_pairs.hpp) built once per call -- the query side's too, not once per
// chunk -- and resident for it. The tables count against MFM_STORE_MAX_FRACTION together with Q; the per-row scratch formula is
// unchanged. A side with blocks is embedded by k_pairs_embed<true>, one without by k_pairs_embed<false>, which reads no block
// argument, so a call without blocks computes what it computed before there were any.
//
// Forms. What a call launches for its tiles is decided once, by pairs_form(): the mean forms (k_pairs_tile), the moments forms
// (mfm_pairs_moments*, mfm_pairs_topk_ucb*; k_pairs_tile_moments of mfm_pairs_ucb.hpp, DESIGN 4.13.1: the spread over the samples
// kept, ranking by mean + beta * std, and after each chunk's merge k_pairs_moments_at for mean and std of the selected pairs), or
// the rank form (mfm_pairs_set_targets, mfm_pairs_rank*; k_pairs_tile_rank of mfm_pairs_rank.hpp, DESIGN 4.13.2: per query chunk
// the values at the chunk's targets, then the count of the admissible candidates that beat each of them; a chunk without targets
// launches nothing, a call without targets or candidates touches no device memory), or the per-sample selecting form
// (mfm_pairs_topk_samples*, mfm_pairs_topk_prob*; k_pairs_tile_samples and k_pairs_vote of mfm_pairs_samples.hpp, DESIGN 4.13.3:
// walk_samples below builds each query chunk's plan and walks it in slices), or the similarity forms (mfm_pairs_sim*,
// mfm_pairs_topk_sim*; k_pairs_tile_sim of mfm_pairs_sim.hpp, DESIGN 4.13.4: the moments forms' walk over embeddings whose bias slot
// holds the rows' normalisation; the one family that a similarity handle, mfm_pairs_create_sim, serves).
// The variational forms (mfm_pairs_moments_vb, mfm_pairs_topk_bound_vb; mfm_pairs_vb.hpp) score a mean-field Gaussian
// posterior instead of samples: score_vb below, which hands its embedding to the query walk of the sample forms (walk_queries).
// The screened top-k (mfm_pairs_topk_screened*, mfm_pairs_screen_scores*; mfm_pairs_screen.hpp): mode 0's list through a
// bf16 contraction, an exact rescoring of its shortlist and a per-row certificate (run_screened below); a bf16 copy of Q is resident
// next to Q and counts in the memory rule.
// The diversified top-k (mfm_pairs_topk_diverse*; mfm_pairs_diverse.hpp): the mean forms' top-k of length `pool` per
// query chunk, left on the device, and greedy maximal marginal relevance over it (run_diverse below); a row-major, pre-normalised
// copy of Q is resident next to Q for the call and counts in the memory rule.
#include "mfm_pairs.hpp"
#include "mfm_pairs_diverse.hpp"
#include "mfm_pairs_rank.hpp"
#include "mfm_pairs_samples.hpp"
#include "mfm_pairs_screen.hpp"
#include "mfm_pairs_sim.hpp"
#include "mfm_pairs_ucb.hpp"
#include "mfm_pairs_vb.hpp"
#include "mfm_samples.hpp"

#include <algorithm>
#include <cmath>
#include <memory>

using namespace mfm;

struct mfm_pairs {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int64_t D = 0, U = 0, I = 0;
  DevBuf<int64_t> q_ptr, c_ptr, e_ptr;
  DevBuf<int32_t> q_idx, c_idx, e_idx;
  DevBuf<double> q_val, c_val;
  // relation blocks of the two sides (0 query, 1 candidates), in the order they were added
  struct Block {
    int64_t off = 0, width = 0, M = 0;
    DevBuf<int64_t> o2b, ptr;
    DevBuf<int32_t> idx;
    DevBuf<double> val;
  };
  std::vector<std::unique_ptr<Block>> blocks[2];
  std::vector<uint8_t> stored[2];  // per side: column j of the model's feature space is stored in its main matrix or in a block
  std::vector<double> cut;         // [cut_S][n_cut], the samples' cutpoints (mode 2)
  int cut_S = 0, n_cut = 0;
  std::vector<int64_t> e_ptr_host;  // (the exclusions of a chunk are counted on the host)
  std::vector<int32_t> e_idx_host;  // (and compared with the targets there)
  bool has_exclude = false;
  // the targets of the rank form: CSR pattern (U, I), columns sorted and unique within a row
  DevBuf<int64_t> t_ptr;
  DevBuf<int32_t> t_idx;
  std::vector<int64_t> t_ptr_host;
  std::vector<int32_t> t_idx_host;
  bool has_targets = false;
  int64_t scratch_bound = (int64_t)256 << 20;
  bool similarity = false;  // made by mfm_pairs_create_sim: the sides may share columns, only the similarity forms run on it
  ~mfm_pairs() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  void use_device() { MFM_HIP_CHECK(hipSetDevice(device)); }
};

static thread_local std::string g_pairs_error;

#define PAIRS_TRY(p) \
  try {              \
    (p)->use_device();
#define PAIRS_CATCH(p)               \
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

void check_csr(int64_t rows, int64_t cols, const int64_t *indptr, const int32_t *indices, const char *what) {
  if (rows < 0 || cols < 0) throw Error(MFM_ERR_INVALID, std::string(what) + ": negative matrix shape");
  if (indptr[0] != 0) throw Error(MFM_ERR_INVALID, std::string(what) + ": indptr[0] must be 0");
  for (int64_t i = 0; i < rows; i++)
    if (indptr[i + 1] < indptr[i]) throw Error(MFM_ERR_INVALID, std::string(what) + ": indptr must be non-decreasing");
  for (int64_t p = 0; p < indptr[rows]; p++)
    if (indices[p] < 0 || indices[p] >= cols) throw Error(MFM_ERR_INVALID, std::string(what) + ": column index out of range");
}

int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

template <class T>
void ensure(DevBuf<T> &b, size_t n) {
  if (b.n < std::max<size_t>(n, 1)) b.alloc(std::max<size_t>(n, 1));
}

// ---- what a call asks for ---------------------------------------------------------------------------------------------------------
// The forms of the C ABI, the variational calls included (the moments and the ranked moments of mfm_pairs_vb.hpp).
enum PairsAsk {
  ASK_SCORES,        // (U, I) values
  ASK_TOPK,          // the k best per query row
  ASK_MOMENTS,       // (U, I) mean and std over the samples
  ASK_UCB,           // the k best by mean + beta * std, with mean and std
  ASK_RANK,          // value and rank of every stored target
  ASK_SAMPLES,       // the k best under each sample, or under each row's own
  ASK_VOTE,          // the n_top candidates most often in the samples' lists
  ASK_SCREENED,      // mode 0's k best through the bf16 screen, certified per row
  ASK_SCREEN_DENSE,  // (U, I) screened values and the per-row bound
  ASK_SIM,           // (U, I) mean and std of the similarity
  ASK_TOPK_SIM,      // the k most similar by mean + beta * std
  ASK_DIVERSE        // k greedy picks by relevance minus redundancy out of the `pool` best
};

// One request: the form, its parameters and its outputs by name. The checked_* functions below build it, with the checks that need
// neither samples nor a device; a field that the form does not use keeps its default.
struct PairsRequest {
  PairsAsk ask;
  int mode = 0;     // the prediction mode; the similarity and the screened forms score under 0
  int metric = -1;  // PAIRS_SIM_*, the similarity forms alone
  int k = 0;
  double beta = 0.0;                    // the ranked moments forms rank by mean + beta * std
  const int32_t *row_sample = nullptr;  // ASK_SAMPLES, [U]: only the list of row u's own sample, outputs [U][k]; null: every sample's, [S][U][k]
  int n_top = 0;                        // ASK_VOTE: idx / value are [U][n_top] indices / probabilities
  int pool = 0;                         // ASK_DIVERSE: the picks come out of the top `pool` of the mean form
  double lam = 0.0;                     // ASK_DIVERSE: g = lam * relevance - (1 - lam) * redundancy
  // the outputs
  double *dense = nullptr;                      // (U, I): the value, the moments forms' mean, the screen's r~
  int64_t *idx = nullptr;                       // the lists: (U, k), or as the per-sample forms lay them out
  double *value = nullptr;
  double *mean = nullptr;                       // (U, k): the moments of the listed pairs
  double *sd = nullptr;                         // (U, k), or (U, I) next to `dense`
  int64_t *target_rank = nullptr;               // ASK_RANK: one entry per stored target in CSR order
  double *target_value = nullptr;
  uint8_t *certified = nullptr;                 // ASK_SCREENED, [U]
  double *bound = nullptr;                      // ASK_SCREEN_DENSE, [U]: E_u
  double *objective = nullptr;                  // ASK_DIVERSE, (U, k): g of each pick
  double *redundancy = nullptr;                 // ASK_DIVERSE, (U, k): the pick's largest similarity with the picks before it

  int list_k() const { return ask == ASK_DIVERSE ? pool : k; }  // the length of the lists the tile kernel selects

  bool dense_form() const { return ask == ASK_SCORES || ask == ASK_MOMENTS || ask == ASK_SCREEN_DENSE || ask == ASK_SIM; }
  bool spread() const { return ask == ASK_MOMENTS || ask == ASK_UCB || sim(); }
  bool sim() const { return ask == ASK_SIM || ask == ASK_TOPK_SIM; }
  bool per_sample() const { return ask == ASK_SAMPLES || ask == ASK_VOTE; }
  bool screened() const { return ask == ASK_SCREENED || ask == ASK_SCREEN_DENSE; }
};

// ---- the steps every driver shares ------------------------------------------------------------------------------------------------
// the sizes every formula of a call reads: S samples (or pseudo-samples) of K factors, padded to KS = 4 KS4
struct PairsDims {
  int S, K, KS, KS4;
  int64_t NK, Ipad, W;
};

PairsDims pairs_dims(const mfm_pairs *p, int S, int K) {
  const int KS = (K + 3) & ~3;
  return {S, K, KS, KS / 4, (int64_t)S * (KS / 4), round_up(std::max<int64_t>(p->I, 1), PAIRS_COL_ALIGN), (p->I + 31) / 32};
}

// the resident part of a call against MFM_STORE_MAX_FRACTION (default 0.5) of the free device memory
bool exceeds_store_fraction(double bytes) {
  size_t free_b = 0, total_b = 0;
  const double frac = env_double("MFM_STORE_MAX_FRACTION", 0.5);
  return hipMemGetInfo(&free_b, &total_b) == hipSuccess && bytes > frac * (double)free_b;
}

// query rows per chunk: what `bound` bytes hold at `per_row` bytes a row, in whole 64-row tiles and never less than one
int64_t chunk_rows(int64_t bound, double per_row, int64_t U) {
  int64_t chunk = (int64_t)std::min<double>((double)bound / per_row, 1e12);
  chunk = std::max<int64_t>(chunk / PAIRS_ROW_ALIGN * PAIRS_ROW_ALIGN, PAIRS_ROW_ALIGN);
  return std::min<int64_t>(chunk, round_up(U, PAIRS_ROW_ALIGN));
}

// steps of `step` candidates that a workgroup takes over the whole candidate side
int64_t candidate_steps(int64_t I, int step) { return (std::max<int64_t>(I, 1) + step - 1) / step; }

// stripes of the candidate walk for a launch of n_tiles row tiles (or plan entries): enough workgroups to fill the device twice, at
// most PAIRS_MAX_STRIPES lists to merge, no empty stripe
struct Stripes {
  int64_t n, steps;
};

Stripes split_stripes(int64_t n_tiles, int64_t steps_total) {
  const int64_t n = std::max<int64_t>(1, std::min<int64_t>({(512 + n_tiles - 1) / n_tiles, steps_total, (int64_t)PAIRS_MAX_STRIPES}));
  const int64_t steps = (steps_total + n - 1) / n;
  return {(steps_total + steps - 1) / steps, steps};
}

// the exclusion bitmask [Uc][W] of the chunk's rows, built in `mask`; null when the chunk excludes nothing
const uint32_t *chunk_mask(mfm_pairs *p, DevBuf<uint32_t> &mask, int64_t u0, int64_t Uc, int64_t W) {
  if (!p->has_exclude || !(p->e_ptr_host[u0 + Uc] > p->e_ptr_host[u0])) return nullptr;
  ensure(mask, (size_t)(Uc * W));
  MFM_HIP_CHECK(hipMemsetAsync(mask.p, 0, (size_t)(Uc * W) * sizeof(uint32_t), p->stream));
  hipLaunchKernelGGL(k_pairs_mask, dim3((unsigned)((Uc + 3) / 4)), dim3(PAIRS_WG), 0, p->stream, p->e_ptr.p, p->e_idx.p, u0, Uc, W, mask.p);
  return mask.p;
}

// a chunk's rows of P and their biases (Asum stays empty where the form sums none)
struct QueryRows {
  DevBuf<double> Pf, Ab, Asum;
};

// a chunk's PairsArgs from the call's: its rows, its share of the grid, its mask; the form's own outputs are the driver's to add
PairsArgs chunk_args(const PairsArgs &call, const QueryRows &q, int64_t u0, int64_t Uc, int64_t Upad, int64_t stripe_len, const uint32_t *mask) {
  PairsArgs a = call;
  a.Pf = q.Pf.p;
  a.Ab = q.Ab.p;
  a.Asum = q.Asum.p;
  a.Upad = Upad;
  a.Uc = Uc;
  a.stripe_len = stripe_len;
  a.mask = mask;
  a.list_rows = Upad;
  a.u0 = u0;
  return a;
}

// A finished (rows, k) list off the device to row `row0` of the caller's arrays: the values straight, the indices through h_idx and
// widened from int32 to int64. Synchronises the stream: whatever else the chunk has queued has arrived too, and the chunk's device and
// host buffers may be reused.
void download_list(hipStream_t s, std::vector<int32_t> &h_idx, const double *d_value, const int32_t *d_idx, int64_t rows, int64_t k, int64_t row0,
                   double *value, int64_t *idx) {
  h_idx.resize((size_t)(rows * k));
  MFM_HIP_CHECK(hipMemcpyAsync(value + (size_t)(row0 * k), d_value, (size_t)(rows * k) * sizeof(double), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), d_idx, (size_t)(rows * k) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MFM_HIP_CHECK(hipStreamSynchronize(s));
  for (int64_t e = 0; e < rows * k; e++) idx[row0 * k + e] = h_idx[(size_t)e];
}

// ---- the forms of the tile kernel ---------------------------------------------------------------------------------------------
// launches a tile kernel with its dynamic LDS, the limit raised once per device where the form needs more than the default
template <auto KERNEL>
void launch_pairs(hipStream_t s, dim3 grid, size_t lds, const PairsArgs &a) {
  static DeviceOnce raised;
  if (lds > 48 * 1024 && raised.need()) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised.mark();
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(PAIRS_WG), lds, s, a);
}

// what becomes of a finished value: written (the scores entry points), selected (the top k), or looked up and counted at the
// targets (the rank form's two launches); PAIRS_SELECT_SAMPLE: selected under one sample per workgroup, by a plan
enum PairsOut { PAIRS_DENSE, PAIRS_SELECT, PAIRS_TARGETS, PAIRS_SELECT_SAMPLE };

template <int MT, int NT, int MODE, bool SPREAD, PairsOut OUT>
void launch_form_mode(hipStream_t s, dim3 grid, const PairsArgs &a) {
  if constexpr (OUT == PAIRS_TARGETS) {
    launch_pairs<k_pairs_tile_rank<MT, NT, MODE, false>>(s, grid, PairsRankLds<false>::BYTES, a);
    MFM_HIP_CHECK(hipGetLastError());
    launch_pairs<k_pairs_tile_rank<MT, NT, MODE, true>>(s, grid, PairsRankLds<true>::BYTES, a);
  } else if constexpr (OUT == PAIRS_SELECT_SAMPLE) {
    launch_pairs<k_pairs_tile_samples<MT, NT, MODE>>(s, grid, PairsSel<MT>::BYTES, a);
  } else {
    constexpr bool DENSE = OUT == PAIRS_DENSE;
    const size_t lds = DENSE ? 0 : PairsSel<MT>::BYTES;
    if constexpr (SPREAD)
      launch_pairs<k_pairs_tile_moments<MT, NT, MODE, DENSE>>(s, grid, lds, a);
    else
      launch_pairs<k_pairs_tile<MT, NT, MODE, DENSE>>(s, grid, lds, a);
  }
}

// the similarity forms (mfm_pairs_sim.hpp): one per tile shape, whatever the metric and the task
template <int MT, int NT, PairsOut OUT>
void launch_form_sim(hipStream_t s, dim3 grid, const PairsArgs &a, int) {
  constexpr bool DENSE = OUT == PAIRS_DENSE;
  launch_pairs<k_pairs_tile_sim<MT, NT, DENSE>>(s, grid, DENSE ? 0 : PairsSel<MT>::BYTES, a);
}

template <int MT, int NT, bool SPREAD, PairsOut OUT>
void launch_form(hipStream_t s, dim3 grid, const PairsArgs &a, int mode) {
  if (mode == 0)
    launch_form_mode<MT, NT, 0, SPREAD, OUT>(s, grid, a);
  else if (mode == 1)
    launch_form_mode<MT, NT, 1, SPREAD, OUT>(s, grid, a);
  else
    launch_form_mode<MT, NT, 2, SPREAD, OUT>(s, grid, a);
}

// The form of a call: a workgroup takes 16 MT query rows and walks its stripe in steps of 64 NT candidates.
struct PairsForm {
  int MT, NT;
  bool spread;  // the moments over the samples (mfm_pairs_ucb.hpp) instead of the mean
  PairsOut out;
  void (*launch)(hipStream_t, dim3, const PairsArgs &, int mode);
  bool sim = false;  // the similarity finish (mfm_pairs_sim.hpp) instead of the score's
  int rows() const { return 16 * MT; }
  int step() const { return 64 * NT; }
};

template <int MT, int NT, bool SPREAD, PairsOut OUT>
PairsForm pairs_form_of() {
  return {MT, NT, SPREAD, OUT, &launch_form<MT, NT, SPREAD, OUT>};
}

template <int MT, int NT, PairsOut OUT>
PairsForm pairs_sim_form_of() {
  return {MT, NT, true, OUT, &launch_form_sim<MT, NT, OUT>, true};
}

// The one table of forms. A selecting form's tile shape follows from k: the per-row buffers of 16 MT rows x (256 / MT + 64)
// candidates must fit the LDS. The moments forms hold MT NT = 4 tiles (their accumulators take twice the registers), the rank
// form has the one shape its target lists are laid out for. The per-sample selecting forms hold one sample's value next to the
// accumulators, as the mean forms' modes 1 and 2 do, and take their shapes. The similarity forms are moments forms with another
// finish and take the moments forms' shapes.
PairsForm pairs_form(const PairsRequest &rq) {
  const bool dense = rq.dense_form();
  const int k = rq.list_k();
  if (rq.sim()) {
    if (dense) return pairs_sim_form_of<2, 2, PAIRS_DENSE>();
    if (k <= 64) return pairs_sim_form_of<4, 1, PAIRS_SELECT>();
    if (k <= 128) return pairs_sim_form_of<2, 2, PAIRS_SELECT>();
    return pairs_sim_form_of<1, 4, PAIRS_SELECT>();
  }
  if (rq.ask == ASK_RANK) return pairs_form_of<4, 2, false, PAIRS_TARGETS>();
  if (rq.per_sample()) {
    if (k <= 64) return pairs_form_of<4, 2, false, PAIRS_SELECT_SAMPLE>();
    if (k <= 128) return pairs_form_of<2, 4, false, PAIRS_SELECT_SAMPLE>();
    return pairs_form_of<1, 8, false, PAIRS_SELECT_SAMPLE>();
  }
  if (!rq.spread()) {
    if (dense) return pairs_form_of<4, 2, false, PAIRS_DENSE>();
    if (k <= 64) return pairs_form_of<4, 2, false, PAIRS_SELECT>();
    if (k <= 128) return pairs_form_of<2, 4, false, PAIRS_SELECT>();
    return pairs_form_of<1, 8, false, PAIRS_SELECT>();
  }
  if (dense) return pairs_form_of<2, 2, true, PAIRS_DENSE>();
  if (k <= 64) return pairs_form_of<4, 1, true, PAIRS_SELECT>();
  if (k <= 128) return pairs_form_of<2, 2, true, PAIRS_SELECT>();
  return pairs_form_of<1, 4, true, PAIRS_SELECT>();
}

void launch_moments_at(hipStream_t s, const PairsArgs &a, int mode, bool sim, const int32_t *out_i, int64_t n, double *mean, double *sd) {
  const dim3 grid((unsigned)((n + PAIRS_WG / 64 - 1) / (PAIRS_WG / 64)));
  if (sim)
    hipLaunchKernelGGL((k_pairs_moments_at<0, PairsFinishSim>), grid, dim3(PAIRS_WG), 0, s, a, out_i, n, mean, sd);
  else if (mode == 0)
    hipLaunchKernelGGL(k_pairs_moments_at<0>, grid, dim3(PAIRS_WG), 0, s, a, out_i, n, mean, sd);
  else if (mode == 1)
    hipLaunchKernelGGL(k_pairs_moments_at<1>, grid, dim3(PAIRS_WG), 0, s, a, out_i, n, mean, sd);
  else
    hipLaunchKernelGGL(k_pairs_moments_at<2>, grid, dim3(PAIRS_WG), 0, s, a, out_i, n, mean, sd);
}

// a target that is also excluded has no rank: refused when the second of the two patterns arrives
void check_targets_not_excluded(const mfm_pairs *p) {
  if (!p->has_targets || !p->has_exclude) return;
  for (int64_t u = 0; u < p->U; u++) {
    const int32_t *tb = p->t_idx_host.data() + p->t_ptr_host[u], *te = p->t_idx_host.data() + p->t_ptr_host[u + 1];
    if (tb == te) continue;
    for (int64_t q = p->e_ptr_host[u]; q < p->e_ptr_host[u + 1]; q++)
      if (std::binary_search(tb, te, p->e_idx_host[(size_t)q]))
        throw Error(MFM_ERR_INVALID, "targets: the pair (query row " + std::to_string(u) + ", candidate " +
                                         std::to_string(p->e_idx_host[(size_t)q]) + ") is also excluded");
  }
}

// ---- the per-sample selecting form (mfm_pairs_samples.hpp) --------------------------------------------------------
static_assert(PAIRS_VOTE_MAX == MFM_PAIRS_VOTE_MAX && PAIRS_VOTE_MAX >= 95 * PAIRS_MAX_K, "the vote's limit as the header states it");

// the checks that need the sample count (before any launch)
void check_per_sample(const PairsRequest &rq, int S, int64_t U) {
  if (rq.row_sample)
    for (int64_t u = 0; u < U; u++)
      if (rq.row_sample[u] < 0 || rq.row_sample[u] >= S)
        throw Error(MFM_ERR_INVALID, "row_sample: query row " + std::to_string(u) + " asks for sample " + std::to_string(rq.row_sample[u]) +
                                         ", the call has " + std::to_string(S));
  if (rq.ask == ASK_VOTE && (int64_t)S * rq.k > PAIRS_VOTE_MAX)
    throw Error(MFM_ERR_INVALID, "the vote takes at most " + std::to_string(PAIRS_VOTE_MAX) + " list entries per query row (samples * k), the call has " +
                                     std::to_string((int64_t)S * rq.k));
}

// The queries in chunks, each chunk's plan in slices (the candidate side is resident: `call`).
// Chunk: its per-row scratch -- P and the biases (all samples, or the row's own with the two maps), the exclusion bitmask, the
// votes and the voted result -- stays under HALF the scratch bound (never less than one 64-row tile). Slice: consecutive plan
// entries whose stripe lists and merged lists fit what the chunk's scratch leaves of the bound (never less than one entry). The
// stripes are chosen per chunk from its entry count, as the other forms choose them from their row tiles. Every list is merged
// under the selection's total order and lands at a place that its (sample, row) alone decides, so neither the bound nor the
// stripes nor the slices change a bit of the results.
template <class Embed>
void walk_samples(mfm_pairs *p, const PairsForm &form, const PairsArgs &call, const PairsRequest &rq, Embed embed) {
  hipStream_t s = p->stream;
  const int S = call.S, k = call.k, KS = call.KS4 * 4, rows = form.rows(), n_top = rq.n_top;
  const int64_t U = p->U, I = call.I, W = call.W;
  const bool own = rq.row_sample != nullptr, vote = rq.ask == ASK_VOTE, masked = p->has_exclude;
  const double per_row = (own ? (double)KS * 8 + 16 : (double)S * KS * 8 + (double)S * 8) + (masked ? (double)W * 4 : 0.0) +
                         (vote ? (double)S * k * 4 + (double)n_top * 12 : 0.0);
  const int64_t chunk = chunk_rows(p->scratch_bound / 2, per_row, U);
  const int64_t steps_total = candidate_steps(I, form.step());
  int n_sort = 2;  // the vote's sort length: the power of two at or above S * k
  while (vote && n_sort < S * k) n_sort <<= 1;

  QueryRows q;
  DevBuf<double> list_v, out_v, res_p;
  DevBuf<int32_t> list_i, out_i, votes, res_i, d_row_of, d_map_s;
  DevBuf<uint32_t> mask;
  DevBuf<PairsPlanEntry> d_plan;
  std::vector<PairsPlanEntry> plan;
  std::vector<int32_t> row_of, map_s, h_idx;
  std::vector<double> h_val;
  std::vector<int64_t> fill((size_t)S);
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    // ---- the chunk's plan (out: the entry's place in its slice, set below) and its rows of P
    plan.clear();
    int64_t Ppad = Upad;
    if (own) {
      // the rows grouped by their sample, a group's rows in row order, every non-empty group padded to whole tiles
      std::fill(fill.begin(), fill.end(), 0);
      for (int64_t u = 0; u < Uc; u++) fill[(size_t)rq.row_sample[u0 + u]]++;
      Ppad = 0;
      for (int g = 0; g < S; g++) {
        const int64_t n_g = fill[(size_t)g];
        fill[(size_t)g] = Ppad;  // (from here on: where the group's next row goes)
        for (int64_t t = 0; t < n_g; t += rows) plan.push_back({Ppad + t, 0, g, (int32_t)std::min<int64_t>(rows, n_g - t)});
        Ppad += round_up(n_g, rows);
      }
      row_of.assign((size_t)Ppad, -1);
      map_s.assign((size_t)Ppad, 0);
      for (int64_t u = 0; u < Uc; u++) row_of[(size_t)fill[(size_t)rq.row_sample[u0 + u]]++] = (int32_t)u;
      for (const PairsPlanEntry &e : plan)
        for (int r = 0; r < rows; r++) map_s[(size_t)e.row0 + r] = e.s;
    } else {
      for (int g = 0; g < S; g++)
        for (int64_t t = 0; t < Uc; t += rows) plan.push_back({t, 0, g, (int32_t)std::min<int64_t>(rows, Uc - t)});
    }
    const int64_t n_e = (int64_t)plan.size();
    if (n_e == 0) continue;
    const Stripes stripes = split_stripes(n_e, steps_total);
    const int64_t n_stripes = stripes.n;
    // slices: what the chunk's own scratch leaves of the bound, in entries
    const double fixed = (own ? (double)Ppad * (KS * 8 + 16) : (double)Upad * S * (KS + 1) * 8) + (masked ? (double)Uc * W * 4 : 0.0) +
                         (vote ? (double)Uc * ((double)S * k * 4 + (double)n_top * 12) : 0.0);
    const double per_entry = (double)(n_stripes + 1) * rows * k * 12 + sizeof(PairsPlanEntry);
    const int64_t slice = std::max<int64_t>(1, (int64_t)std::min<double>(((double)p->scratch_bound - fixed) / per_entry, (double)n_e));
    for (int64_t e = 0; e < n_e; e++) plan[(size_t)e].out = (e % slice) * rows;
    d_plan.upload(plan);
    if (own) {
      d_row_of.upload(row_of);
      d_map_s.upload(map_s);
    }
    // ---- P, the mask
    ensure(q.Pf, (size_t)(Ppad * (own ? (int64_t)KS : (int64_t)S * KS)));
    ensure(q.Ab, (size_t)(own ? Ppad : Upad * S));
    embed(0, u0, Uc, Ppad, q.Pf.p, q.Ab.p, own ? d_row_of.p : nullptr, own ? d_map_s.p : nullptr);
    MFM_HIP_CHECK(hipGetLastError());
    PairsArgs a = chunk_args(call, q, u0, Uc, Upad, stripes.steps * form.step(), chunk_mask(p, mask, u0, Uc, W));
    a.p_stride = own ? (int64_t)call.KS4 : call.NK;
    a.row_of = own ? d_row_of.p : nullptr;
    a.list_rows = slice * rows;
    ensure(list_v, (size_t)(n_stripes * slice * rows * k));
    ensure(list_i, (size_t)(n_stripes * slice * rows * k));
    ensure(out_v, (size_t)(slice * rows * k));
    ensure(out_i, (size_t)(slice * rows * k));
    a.list_v = list_v.p;
    a.list_i = list_i.p;
    if (vote) ensure(votes, (size_t)(Uc * S * k));
    for (int64_t e0 = 0; e0 < n_e; e0 += slice) {
      const int64_t E = std::min(slice, n_e - e0), L = E * rows;
      a.plan = d_plan.p + e0;
      if (I > 0) {
        form.launch(s, dim3((unsigned)E, (unsigned)n_stripes), a, rq.mode);
        MFM_HIP_CHECK(hipGetLastError());
      }
      hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)L), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, a.list_rows, k,
                         out_v.p, out_i.p);
      MFM_HIP_CHECK(hipGetLastError());
      if (vote) {  // the lists stay on the device
        hipLaunchKernelGGL(k_pairs_votes_put, dim3((unsigned)E), dim3(PAIRS_WG), 0, s, a.plan, out_i.p, k, S, votes.p);
        MFM_HIP_CHECK(hipGetLastError());
        continue;
      }
      h_idx.resize((size_t)(L * k));
      h_val.resize((size_t)(L * k));
      MFM_HIP_CHECK(hipMemcpyAsync(h_val.data(), out_v.p, (size_t)(L * k) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), out_i.p, (size_t)(L * k) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      // a list goes where its (sample, row) says: [s][u][k], or -- the row's own sample -- [u][k]
      for (int64_t e = e0; e < e0 + E; e++) {
        const PairsPlanEntry &pe = plan[(size_t)e];
        for (int r = 0; r < pe.rows; r++) {
          const int64_t row = own ? (int64_t)row_of[(size_t)pe.row0 + r] : pe.row0 + r;
          const size_t o = (size_t)((own ? (int64_t)0 : (int64_t)pe.s * U) + u0 + row) * k, l = (size_t)(pe.out + r) * k;
          for (int j = 0; j < k; j++) {
            rq.idx[o + j] = h_idx[l + j];
            rq.value[o + j] = h_val[l + j];
          }
        }
      }
    }
    if (vote) {
      ensure(res_i, (size_t)(Uc * n_top));
      ensure(res_p, (size_t)(Uc * n_top));
      const size_t lds = (size_t)n_sort * sizeof(int);
      static DeviceOnce raised;
      if (lds > 48 * 1024 && raised.need()) {
        MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k_pairs_vote, hipFuncAttributeMaxDynamicSharedMemorySize, PAIRS_VOTE_MAX * (int)sizeof(int)));
        raised.mark();
      }
      hipLaunchKernelGGL(k_pairs_vote, dim3((unsigned)Uc), dim3(PAIRS_WG), lds, s, votes.p, S * k, n_sort, S, n_top, res_i.p, res_p.p);
      MFM_HIP_CHECK(hipGetLastError());
      download_list(s, h_idx, res_p.p, res_i.p, Uc, n_top, u0, rq.value, rq.idx);
    }
    MFM_HIP_CHECK(hipStreamSynchronize(s));
  }
}

// ---- the screened top-k (mfm_pairs_screen.hpp) -------------------------------------------------------------------
// the bf16 copy of Q, its norms and flags: what a screened call keeps resident beyond a plain one
double screen_q_bytes(int64_t Ipad, int64_t NK) {
  const int64_t Ipb = round_up(Ipad, SCREEN_COL_ALIGN), NC = round_up(NK * 4, SCREEN_INNER) / SCREEN_INNER;
  return (double)Ipb * NC * SCREEN_INNER * 2 + (double)Ipb * 12;
}

template <auto KERNEL>
void launch_screen(hipStream_t s, dim3 grid, size_t lds, const ScreenArgs &sa) {
  static DeviceOnce raised;
  if (lds > 48 * 1024 && raised.need()) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised.mark();
  }
  hipLaunchKernelGGL(KERNEL, grid, dim3(PAIRS_WG), lds, s, sa);
}

// The form of a screened call: the shortlist length k_s picks the rows per tile by PairsSel's table, the dense diagnostic takes 64.
struct ScreenForm {
  int MT;
  void (*launch)(hipStream_t, dim3, const ScreenArgs &);
  int rows() const { return 16 * MT; }
  int step() const { return 64 * (16 / MT); }
};

template <int MT, bool DENSE>
ScreenForm screen_form_of() {
  return {MT, [](hipStream_t s, dim3 grid, const ScreenArgs &sa) {
            launch_screen<k_screen_tile<MT, DENSE>>(s, grid, (DENSE ? 0 : PairsSel<MT>::BYTES) + screen_stage_bytes<MT>(), sa);
          }};
}

ScreenForm screen_form(bool dense, int ks) {
  if (dense) return screen_form_of<4, true>();
  if (ks <= 64) return screen_form_of<4, false>();
  if (ks <= 128) return screen_form_of<2, false>();
  return screen_form_of<1, false>();
}

// The queries in chunks against the resident candidate side of `call` (mode 0). Per chunk: embed and pack P, screen into the
// stripes' lists of k_s = min(256, max(64, 2 k)) entries, merge, rescore the merged list's first k_s - 1 entries exactly, finish.
// Scratch per query row: run_pairs' mean-form terms with k_s for k, plus the bf16 P, the norm and flag, the exact values and the
// outputs. The rows that come back uncertified are the caller's to send through mfm_pairs_topk.
template <class Embed>
void run_screened(mfm_pairs *p, const PairsArgs &call, const PairsRequest &rq, Embed embed) {
  hipStream_t s = p->stream;
  const bool is_dense = rq.dense_form();
  const int k = rq.k, S = call.S, KS = call.KS4 * 4, ks = is_dense ? 0 : std::min(256, std::max(64, 2 * k));
  const int64_t U = p->U, I = call.I, W = call.W, NK = call.NK, Ipad = call.Ipad, L = NK * 4;
  const int64_t Lp = round_up(L, SCREEN_INNER), Ipb = round_up(Ipad, SCREEN_COL_ALIGN);
  const int NC = (int)(Lp / SCREEN_INNER);
  const ScreenForm form = screen_form(is_dense, ks);
  const double per_row = (double)S * KS * 8 + (double)(S + 1) * 8 + (double)Lp * 2 + 12 +
                         (is_dense ? (double)I * 8 + 8
                                   : (p->has_exclude ? (double)W * 4 : 0.0) + (double)(PAIRS_MAX_STRIPES + 2) * ks * 12 + (double)k * 12 + 1);
  const int64_t chunk = chunk_rows(p->scratch_bound, per_row, U);
  const int64_t steps_total = candidate_steps(I, form.step());

  // ---- candidate side, once: the bf16 copy, the norms, the flags and the two maxima
  DevBuf<screen_u4> Qb, Pb;
  DevBuf<double> qn, cmax, pn;
  DevBuf<int32_t> qflag, cand_flag, pflag;
  Qb.alloc((size_t)std::max<int64_t>(Ipb / 16 * NC * 64, 1));
  qn.alloc((size_t)Ipb);
  qflag.alloc((size_t)Ipb);
  cmax.alloc(2);
  cand_flag.alloc_zero(1, s);
  hipLaunchKernelGGL(k_screen_pack, dim3((unsigned)(Ipb / 16)), dim3(PAIRS_WG), 0, s, call.Qf, NK, Ipad / 16, NC, call.Bsum, Qb.p, qn.p, qflag.p,
                     cand_flag.p);
  hipLaunchKernelGGL(k_screen_cand_max, dim3(1), dim3(PAIRS_WG), 0, s, (const double *)qn.p, call.Bsum, I, cmax.p);
  MFM_HIP_CHECK(hipGetLastError());

  QueryRows q;
  DevBuf<double> list_v, sl_v, ex_v, out_v, d_dense, d_E;
  DevBuf<int32_t> list_i, sl_i, out_i;
  DevBuf<uint32_t> mask;
  DevBuf<uint8_t> d_cert;
  std::vector<int32_t> h_idx;
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    ensure(q.Pf, (size_t)(Upad * NK * 4));
    ensure(q.Ab, (size_t)(Upad * S));
    ensure(q.Asum, (size_t)Upad);
    ensure(Pb, (size_t)(Upad / 16 * NC * 64));
    ensure(pn, (size_t)Upad);
    ensure(pflag, (size_t)Upad);
    embed(0, u0, Uc, Upad, q.Pf.p, q.Ab.p);
    hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)((Upad + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, q.Ab.p, S, Upad, q.Asum.p);
    hipLaunchKernelGGL(k_screen_pack, dim3((unsigned)(Upad / 16)), dim3(PAIRS_WG), 0, s, (const double *)q.Pf.p, NK, Upad / 16, NC,
                       (const double *)q.Asum.p, Pb.p, pn.p, pflag.p, (int32_t *)nullptr);
    MFM_HIP_CHECK(hipGetLastError());
    const int64_t n_qt = Upad / form.rows();
    const Stripes stripes = split_stripes(n_qt, steps_total);
    const int64_t n_stripes = stripes.n;
    const dim3 grid((unsigned)n_qt, (unsigned)n_stripes);
    ScreenArgs sa;
    sa.a = chunk_args(call, q, u0, Uc, Upad, stripes.steps * form.step(), is_dense ? nullptr : chunk_mask(p, mask, u0, Uc, W));
    sa.a.k = ks;
    sa.Pb = Pb.p;
    sa.Qb = Qb.p;
    sa.NC = NC;
    ScreenBound sb;
    sb.pnorm = pn.p;
    sb.pflag = pflag.p;
    sb.cand_flag = cand_flag.p;
    sb.cmax = cmax.p;
    sb.Asum = q.Asum.p;
    sb.w0sum = call.w0sum;
    sb.eps = screen_eps(Lp);
    sb.L = (double)L;
    sb.S = S;
    if (is_dense) {
      ensure(d_dense, (size_t)(Uc * I));
      ensure(d_E, (size_t)Uc);
      sa.a.dense = d_dense.p;
      form.launch(s, grid, sa);
      hipLaunchKernelGGL(k_screen_bound, dim3((unsigned)((Uc + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, sb, Uc, d_E.p);
      MFM_HIP_CHECK(hipGetLastError());
      MFM_HIP_CHECK(hipMemcpyAsync(rq.dense + (size_t)u0 * I, d_dense.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(rq.bound + u0, d_E.p, (size_t)Uc * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      continue;
    }
    ensure(list_v, (size_t)(n_stripes * Upad * ks));
    ensure(list_i, (size_t)(n_stripes * Upad * ks));
    ensure(sl_v, (size_t)(Uc * ks));
    ensure(sl_i, (size_t)(Uc * ks));
    ensure(ex_v, (size_t)(Uc * ks));
    ensure(out_v, (size_t)(Uc * k));
    ensure(out_i, (size_t)(Uc * k));
    ensure(d_cert, (size_t)Uc);
    sa.a.list_v = list_v.p;
    sa.a.list_i = list_i.p;
    if (I > 0) {
      form.launch(s, grid, sa);
      MFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)Uc), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, Upad, ks, sl_v.p,
                       sl_i.p);
    const int64_t waves = Uc * ((ks + 15) / 16);
    hipLaunchKernelGGL(k_screen_rescore, dim3((unsigned)((waves + 3) / 4)), dim3(PAIRS_WG), 0, s, sa.a, (const int32_t *)sl_i.p, ks, ks - 1, ex_v.p);
    hipLaunchKernelGGL(k_screen_finish, dim3((unsigned)((Uc + 3) / 4)), dim3(PAIRS_WG), 0, s, (const double *)sl_v.p, (const int32_t *)sl_i.p,
                       (const double *)ex_v.p, ks, k, Uc, sb, out_v.p, out_i.p, d_cert.p);
    MFM_HIP_CHECK(hipGetLastError());
    MFM_HIP_CHECK(hipMemcpyAsync(rq.certified + u0, d_cert.p, (size_t)Uc, hipMemcpyDeviceToHost, s));
    download_list(s, h_idx, out_v.p, out_i.p, Uc, k, u0, rq.value, rq.idx);
  }
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- the diversified top-k (mfm_pairs_diverse.hpp) ---------------------------------------------------------------
// the row-major pre-normalised copy of Q: what a diversified call keeps resident beyond a plain one (valid candidates only)
double diverse_q_bytes(int64_t I, int64_t NK) { return (double)I * (double)div_padded_length(NK * 4) * sizeof(double); }

// The queries in chunks against the resident candidate side of `call` (call.k = the pool length M; `form`: the mean form that
// mfm_pairs_topk takes for k = M). Once, before the first chunk: k_div_pack. Per chunk: embed P, the form's launch and the merge exactly
// as walk_queries queues them for a top-k of M -- the pool, which stays on the device --, then k_div_select, one workgroup per query
// row, and the download of the k picks. Scratch per query row: walk_queries' selecting terms with M for k, plus the four outputs.
// Qh lives for this call alone and is freed when it returns.
template <class Embed>
void run_diverse(mfm_pairs *p, const PairsForm &form, const PairsArgs &call, const PairsRequest &rq, Embed embed) {
  hipStream_t s = p->stream;
  const int S = call.S, KS = call.KS4 * 4, M = rq.pool, k = rq.k;
  const int64_t U = p->U, I = call.I, W = call.W, L = call.NK * 4, Lpad = div_padded_length(L);
  const double per_row = (double)S * KS * 8 + (double)(S + 1) * 8 + (p->has_exclude ? (double)W * 4 : 0.0) +
                         (double)(PAIRS_MAX_STRIPES + 1) * M * 12 + (double)k * 28;
  const int64_t chunk = chunk_rows(p->scratch_bound, per_row, U);
  const int64_t steps_total = candidate_steps(I, form.step());

  DevBuf<double> Qh;
  Qh.alloc((size_t)std::max<int64_t>(I * Lpad, 1));
  if (I > 0 && L > 0) {
    hipLaunchKernelGGL(k_div_pack, dim3((unsigned)((I + PAIRS_WG - 1) / PAIRS_WG), (unsigned)S), dim3(PAIRS_WG), 0, s, call.Qf, call.NK, call.KS4,
                       S, I, Lpad, Qh.p);
    MFM_HIP_CHECK(hipGetLastError());
  }
  const size_t lds = div_lds_bytes((int)round_up(M, 16));
  static DeviceOnce raised;
  if (lds > 48 * 1024 && raised.need()) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k_div_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)div_lds_bytes(DIV_MAX_POOL)));
    raised.mark();
  }

  QueryRows q;
  DevBuf<double> list_v, pool_v, out_v, out_g, out_r;
  DevBuf<int32_t> list_i, pool_i, out_i;
  DevBuf<uint32_t> mask;
  std::vector<int32_t> h_idx;
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    ensure(q.Pf, (size_t)(Upad * call.NK * 4));
    ensure(q.Ab, (size_t)(Upad * S));
    ensure(q.Asum, (size_t)Upad);
    embed(0, u0, Uc, Upad, q.Pf.p, q.Ab.p);
    hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)((Upad + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, q.Ab.p, S, Upad, q.Asum.p);
    MFM_HIP_CHECK(hipGetLastError());
    const int64_t n_qt = Upad / form.rows();
    const Stripes stripes = split_stripes(n_qt, steps_total);
    const int64_t n_stripes = stripes.n;
    PairsArgs a = chunk_args(call, q, u0, Uc, Upad, stripes.steps * form.step(), chunk_mask(p, mask, u0, Uc, W));
    ensure(list_v, (size_t)(n_stripes * Upad * M));
    ensure(list_i, (size_t)(n_stripes * Upad * M));
    ensure(pool_v, (size_t)(Uc * M));
    ensure(pool_i, (size_t)(Uc * M));
    a.list_v = list_v.p;
    a.list_i = list_i.p;
    if (I > 0) {
      form.launch(s, dim3((unsigned)n_qt, (unsigned)n_stripes), a, rq.mode);
      MFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)Uc), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, Upad, M, pool_v.p,
                       pool_i.p);
    MFM_HIP_CHECK(hipGetLastError());
    ensure(out_i, (size_t)(Uc * k));
    ensure(out_v, (size_t)(Uc * k));
    ensure(out_g, (size_t)(Uc * k));
    ensure(out_r, (size_t)(Uc * k));
    DivArgs da;
    da.Qh = Qh.p;
    da.Lpad = Lpad;
    da.pool_v = pool_v.p;
    da.pool_i = pool_i.p;
    da.M = M;
    da.k = k;
    da.S = S;
    da.lam = rq.lam;
    da.out_i = out_i.p;
    da.out_v = out_v.p;
    da.out_g = out_g.p;
    da.out_r = out_r.p;
    hipLaunchKernelGGL(k_div_select, dim3((unsigned)Uc), dim3(PAIRS_WG), lds, s, da);
    MFM_HIP_CHECK(hipGetLastError());
    MFM_HIP_CHECK(hipMemcpyAsync(rq.objective + (size_t)u0 * k, out_g.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipMemcpyAsync(rq.redundancy + (size_t)u0 * k, out_r.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    download_list(s, h_idx, out_v.p, out_i.p, Uc, k, u0, rq.value, rq.idx);
  }
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

// ---- the query walk that the sample forms and the variational forms share --------------------------------------------------------
// The queries in chunks against the resident candidate side of `call`. Per chunk: embed P (and sum its biases where the candidate
// side has sums), then what the form does with a value -- the targets' values and ranks (a chunk without targets launches nothing);
// or the dense values; or the stripes' lists, their merge, mean and std of the merged pairs where the form has a spread, and the
// download. What depends on where the model comes from is passed in: `embed` puts a side's rows into P and the biases, `moments_at`
// computes mean and std of listed pairs; the form carries its launch. Scratch per query row: P and the biases, the exclusion bitmask,
// the outputs, and for a selecting form the per-stripe lists at the most stripes a launch can have.
template <class Embed, class MomentsAt>
void walk_queries(mfm_pairs *p, const PairsForm &form, const PairsArgs &call, const PairsRequest &rq, Embed embed, MomentsAt moments_at) {
  hipStream_t s = p->stream;
  const int S = call.S, KS = call.KS4 * 4, k = call.k;
  const int64_t U = p->U, I = call.I, W = call.W;
  const bool is_dense = form.out == PAIRS_DENSE, targets = form.out == PAIRS_TARGETS, bias_sums = call.Bsum != nullptr;
  const double per_row = (double)S * KS * 8 + (double)(S + 1) * 8 + (p->has_exclude && !is_dense ? (double)W * 4 : 0.0) +
                         (is_dense  ? (double)I * 8
                          : targets ? (double)PAIRS_RANK_MAX_T * 12  // (the targets' values and ranks)
                                    : (double)(PAIRS_MAX_STRIPES + 1) * k * 12) +
                         // (the second dense output / mean and std of the lists)
                         (!form.spread ? 0.0 : is_dense ? (double)I * 8 : (double)k * 16);
  const int64_t chunk = chunk_rows(p->scratch_bound, per_row, U);
  const int64_t steps_total = candidate_steps(I, form.step());

  QueryRows q;
  DevBuf<double> list_v, out_v, d_dense, d_dense_std, out_m, out_s, t_val;
  DevBuf<int32_t> list_i, out_i, t_rank;
  DevBuf<uint32_t> mask;
  std::vector<int32_t> h_idx;
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    const int64_t tbase = targets ? p->t_ptr_host[u0] : 0, n_t = targets ? p->t_ptr_host[u0 + Uc] - tbase : 0;
    if (targets && n_t == 0) continue;
    ensure(q.Pf, (size_t)(Upad * call.NK * 4));
    ensure(q.Ab, (size_t)(Upad * S));
    embed(0, u0, Uc, Upad, q.Pf.p, q.Ab.p);
    if (bias_sums) {
      ensure(q.Asum, (size_t)Upad);
      hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)((Upad + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, q.Ab.p, S, Upad, q.Asum.p);
    }
    MFM_HIP_CHECK(hipGetLastError());
    const int64_t n_qt = Upad / form.rows();
    const Stripes stripes = split_stripes(n_qt, steps_total);
    const int64_t n_stripes = stripes.n;
    const dim3 grid((unsigned)n_qt, (unsigned)n_stripes);
    PairsArgs a = chunk_args(call, q, u0, Uc, Upad, stripes.steps * form.step(), is_dense ? nullptr : chunk_mask(p, mask, u0, Uc, W));
    if (targets) {
      ensure(t_val, (size_t)n_t);
      ensure(t_rank, (size_t)n_t);
      a.tptr = p->t_ptr.p;
      a.tidx = p->t_idx.p;
      a.tval = t_val.p;
      a.trank = t_rank.p;
      a.tbase = tbase;
      MFM_HIP_CHECK(hipMemsetAsync(t_rank.p, 0, (size_t)n_t * sizeof(int32_t), s));
      form.launch(s, grid, a, rq.mode);
      MFM_HIP_CHECK(hipGetLastError());
      download_list(s, h_idx, t_val.p, t_rank.p, n_t, 1, tbase, rq.target_value, rq.target_rank);
      continue;
    }
    if (is_dense) {
      ensure(d_dense, (size_t)(Uc * I));
      a.dense = d_dense.p;
      if (form.spread) {
        ensure(d_dense_std, (size_t)(Uc * I));
        a.dense_std = d_dense_std.p;
      }
      form.launch(s, grid, a, rq.mode);
      MFM_HIP_CHECK(hipGetLastError());
      if (form.spread)
        MFM_HIP_CHECK(hipMemcpyAsync(rq.sd + (size_t)u0 * I, d_dense_std.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(rq.dense + (size_t)u0 * I, d_dense.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      continue;
    }
    ensure(list_v, (size_t)(n_stripes * Upad * k));
    ensure(list_i, (size_t)(n_stripes * Upad * k));
    ensure(out_v, (size_t)(Uc * k));
    ensure(out_i, (size_t)(Uc * k));
    a.list_v = list_v.p;
    a.list_i = list_i.p;
    if (I > 0) {
      form.launch(s, grid, a, rq.mode);
      MFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)Uc), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, Upad, k,
                       out_v.p, out_i.p);
    MFM_HIP_CHECK(hipGetLastError());
    if (form.spread) {
      ensure(out_m, (size_t)(Uc * k));
      ensure(out_s, (size_t)(Uc * k));
      moments_at(a, out_i.p, Uc * k, out_m.p, out_s.p);
      MFM_HIP_CHECK(hipGetLastError());
      MFM_HIP_CHECK(hipMemcpyAsync(rq.mean + (size_t)u0 * k, out_m.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(rq.sd + (size_t)u0 * k, out_s.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    download_list(s, h_idx, out_v.p, out_i.p, Uc, k, u0, rq.value, rq.idx);
  }
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

// The candidate side, embedded once and resident for the call (Bsum only where the form sums the biases: the similarity finish and
// the variational forms read the per-sample slots alone, Asum / Bsum stay null), and what every launch of the call reads of it and
// of the request; the model's own fields are its driver's to add, a chunk adds its own.
struct Candidates {
  DevBuf<double> Qf, Bb, Bsum;
};

template <class Embed>
PairsArgs embed_candidates(mfm_pairs *p, const PairsDims &d, const PairsRequest &rq, bool bias_sums, Embed embed, Candidates &c) {
  c.Qf.alloc((size_t)std::max<int64_t>(d.Ipad * d.NK * 4, 1));
  c.Bb.alloc((size_t)d.Ipad * d.S);
  if (bias_sums) c.Bsum.alloc((size_t)d.Ipad);
  embed(1, (int64_t)0, p->I, d.Ipad, c.Qf.p, c.Bb.p);
  if (bias_sums)
    hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)(d.Ipad / PAIRS_WG)), dim3(PAIRS_WG), 0, p->stream, c.Bb.p, d.S, d.Ipad, c.Bsum.p);
  MFM_HIP_CHECK(hipGetLastError());
  PairsArgs call;
  call.Qf = c.Qf.p;
  call.NK = d.NK;
  call.p_stride = d.NK;
  call.q_stride = d.NK;
  call.KS4 = d.KS4;
  call.S = d.S;
  call.Bb = c.Bb.p;
  call.Bsum = c.Bsum.p;
  call.beta = rq.beta;
  call.Ipad = d.Ipad;
  call.I = p->I;
  call.W = d.W;
  call.k = rq.list_k();
  return call;
}

// A similarity handle's sides may share columns: the score's split into per-side terms and one contraction is wrong there, so every
// scoring form is refused on it, before the samples are looked at.
void refuse_similarity_handle(const mfm_pairs *p) {
  if (p->similarity)
    throw Error(MFM_ERR_INVALID, "this is a similarity handle (mfm_pairs_create_sim): its sides may share columns, which the pair score's "
                                 "decomposition does not allow; it serves mfm_pairs_sim* and mfm_pairs_topk_sim* only");
}

// ---- the sample forms ------------------------------------------------------------------------------------------------------------
// The whole call over the samples of `v` (mfm_samples.hpp): the checks that need the samples, the memory rule, the block tables and
// the candidate side, then the walk the request names. The similarity forms (rq.metric, mode 0) are moments forms whose embeddings
// carry the normalisation in the bias slot and sum no bias; everything else is the moments call's.
void run_pairs(mfm_pairs *p, const SampleView &v, const PairsRequest &rq) {
  const int S = v.count(), mode = rq.mode, k = rq.k, sim = rq.metric;
  if (v.device != p->device) throw Error(MFM_ERR_INVALID, "pair design and sample store live on different devices");
  if (v.D != p->D) throw Error(MFM_ERR_INVALID, "feature size mismatch!");
  // a store's device-to-device copies (training stream) must be complete: this stream waits for the latest one's event
  if (v.pushed) MFM_HIP_CHECK(hipStreamWaitEvent(p->stream, v.pushed, 0));
  if (S > 65535) throw Error(MFM_ERR_INVALID, "at most 65535 samples per call");
  if (mode != 0 && mode != 1 && mode != 2)
    throw Error(MFM_ERR_INVALID, "bad prediction mode (0: mean score, 1: mean Phi(score), 2: mean expected class index of the ordered probit)");
  if (mode == 2) {
    if (p->n_cut < 1) throw Error(MFM_ERR_INVALID, "mode 2 needs the samples' cutpoints (mfm_pairs_set_cutpoints), at least one per sample");
    if (p->cut_S != S)
      throw Error(MFM_ERR_INVALID, "mode 2: cutpoints were set for " + std::to_string(p->cut_S) + " samples, the call has " + std::to_string(S));
  }
  const bool is_dense = rq.dense_form(), targets = rq.ask == ASK_RANK;
  if (!is_dense && !targets && (k < 1 || k > PAIRS_MAX_K)) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  // the form of the call, decided here once: the scratch per query row, the stripes, the grid and the launch all read it
  const PairsForm form = pairs_form(rq);
  const int64_t U = p->U, I = p->I, D = p->D;
  if (rq.per_sample()) check_per_sample(rq, S, U);
  if (U == 0 || (is_dense && I == 0)) return;
  if (targets && (I == 0 || !p->has_targets)) return;
  hipStream_t s = p->stream;
  const PairsDims d = pairs_dims(p, S, v.K);
  const int K = d.K, KS = d.KS;

  // ---- the memory rule: Q and every block table resident, the query scratch bounded
  const double q_bytes =
      ((double)d.Ipad * S * KS + (double)d.Ipad * (S + 1)) * sizeof(double) + (rq.screened() ? screen_q_bytes(d.Ipad, d.NK) : 0.0) +
      (rq.ask == ASK_DIVERSE ? diverse_q_bytes(I, d.NK) : 0.0);
  double t_bytes[2] = {0.0, 0.0};
  for (int side = 0; side < 2; side++)
    for (auto &b : p->blocks[side]) t_bytes[side] += (double)b->M * S * (KS + 2) * sizeof(double);
  if (exceeds_store_fraction(q_bytes + t_bytes[0] + t_bytes[1])) {
    if (t_bytes[0] + t_bytes[1] == 0.0)
      throw Error(MFM_ERR_RUNTIME, "pair scoring: the candidate side's embedding (" + std::to_string((int64_t)(q_bytes / 1048576.0)) +
                                       " MB for all samples) exceeds MFM_STORE_MAX_FRACTION of the free device memory; "
                                       "score fewer samples or fewer candidates per call");
    const auto mb = [](double b) { return std::to_string((int64_t)(b / 1048576.0)) + " MB"; };
    const char *large = q_bytes >= t_bytes[0] && q_bytes >= t_bytes[1] ? "the candidate side's embedding"
                        : t_bytes[0] >= t_bytes[1]                     ? "the query side's block tables"
                                                                       : "the candidate side's block tables";
    throw Error(MFM_ERR_RUNTIME, "pair scoring: the candidate side's embedding (" + mb(q_bytes) + "), the query side's block tables (" +
                                     mb(t_bytes[0]) + ") and the candidate side's block tables (" + mb(t_bytes[1]) +
                                     ") for all samples together exceed MFM_STORE_MAX_FRACTION of the free device memory; the largest part is " +
                                     large + ": score fewer samples, fewer candidates or smaller blocks per call");
  }

  // ---- the samples' pointers and w0
  DevBuf<const double *> d_wv;
  DevBuf<double> d_w0;
  d_wv.upload(v.wv);
  d_w0.upload(v.w0);
  double w0sum = 0.0;
  for (int i = 0; i < S; i++) w0sum += v.w0[i];

  DevBuf<double> d_cut;
  if (mode == 2) d_cut.upload(p->cut);

  // ---- the block tables of both sides, once per call
  std::vector<DevBuf<double>> tables[2];
  DevBuf<PairsBlockRef> d_blk[2];
  for (int side = 0; side < 2; side++) {
    std::vector<PairsBlockRef> refs;
    for (auto &b : p->blocks[side]) {
      const size_t SM = (size_t)S * (size_t)b->M;
      tables[side].emplace_back();
      DevBuf<double> &t = tables[side].back();
      t.alloc(std::max<size_t>(SM * (size_t)(KS + 2), 1));
      PairsBlockRef ref;
      ref.o2b = b->o2b.p;
      ref.T = t.p;
      ref.lin = t.p + SM * (size_t)KS;
      ref.vv = t.p + SM * (size_t)(KS + 1);
      ref.M = b->M;
      refs.push_back(ref);
      if (b->M > 0) {
        const auto launch = [&](auto kernel) {
          hipLaunchKernelGGL(kernel, dim3((unsigned)((b->M + PAIRS_WG - 1) / PAIRS_WG), (unsigned)S), dim3(PAIRS_WG), 0, s, b->ptr.p,
                             b->idx.p, b->val.p, b->M, b->off, (const double *const *)d_wv.p, D, K, KS, t.p, t.p + SM * (size_t)KS,
                             t.p + SM * (size_t)(KS + 1));
        };
        sim >= 0 ? launch(k_pairs_embed_block<true>) : launch(k_pairs_embed_block<false>);
        MFM_HIP_CHECK(hipGetLastError());
      }
    }
    if (!refs.empty()) d_blk[side].upload(refs);
  }
  // rows [r0, r0 + R) of a side (0 query, 1 candidates) into Pf and the biases: a side with blocks gathers from its tables, one
  // without takes the instantiation that reads no block argument
  // (map_row / map_s: the row -> sample plan's flavour, one launch row per row of P under its own sample)
  const auto embed = [&](int side, int64_t r0, int64_t R, int64_t Rpad, double *Pf, double *bias, const int32_t *map_row = nullptr,
                         const int32_t *map_s = nullptr) {
    const dim3 grid((unsigned)((Rpad + PAIRS_WG - 1) / PAIRS_WG), map_row ? 1u : (unsigned)S);
    const bool rel = !p->blocks[side].empty();
    const PairsBlockRef *blk = rel ? (const PairsBlockRef *)d_blk[side].p : nullptr;
    const int n_blk = (int)p->blocks[side].size();
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(PAIRS_WG), 0, s, side ? p->c_ptr.p : p->q_ptr.p, side ? p->c_idx.p : p->q_idx.p,
                         side ? p->c_val.p : p->q_val.p, r0, R, Rpad, (const double *const *)d_wv.p, D, K, KS, S, blk, n_blk, Pf, bias, map_row,
                         map_s);
    };
    if (sim == PAIRS_SIM_COSINE)  // (the bias slot gets the rows' 1 / norm, or 1.0: mfm_pairs_sim.hpp)
      rel ? launch(k_pairs_embed<true, false, 1>) : launch(k_pairs_embed<false, false, 1>);
    else if (sim == PAIRS_SIM_DOT)
      rel ? launch(k_pairs_embed<true, false, 2>) : launch(k_pairs_embed<false, false, 2>);
    else if (map_row)
      rel ? launch(k_pairs_embed<true, true>) : launch(k_pairs_embed<false, true>);
    else
      rel ? launch(k_pairs_embed<true, false>) : launch(k_pairs_embed<false, false>);
  };

  Candidates cand;
  PairsArgs call = embed_candidates(p, d, rq, sim < 0, embed, cand);
  call.w0s = d_w0.p;
  call.w0sum = w0sum;
  call.cut = mode == 2 ? d_cut.p : nullptr;
  call.n_cut = mode == 2 ? p->n_cut : 0;
  if (rq.per_sample())
    walk_samples(p, form, call, rq, embed);
  else if (rq.screened())
    run_screened(p, call, rq, embed);
  else if (rq.ask == ASK_DIVERSE)
    run_diverse(p, form, call, rq, embed);
  else
    walk_queries(p, form, call, rq, embed, [&](const PairsArgs &a, const int32_t *out_i, int64_t n, double *mean, double *sd) {
      launch_moments_at(s, a, mode, form.sim, out_i, n, mean, sd);
    });
}

// ---- the variational forms (mfm_pairs_vb.hpp) ----------------------------------------------------------------------
// Analytic mean and standard deviation of the score of every pair under the posterior N(w0, w0_var), N(w, w_var), N(V, V_var): five
// pseudo-samples of width KS through the per-sample contraction, ASK_MOMENTS or ASK_UCB. The memory rule, the chunks, the stripes and
// the merge are walk_queries', with S = 5 in every formula; the tile shapes are the moments forms' (MT NT = 4).
template <int MT, int NT, PairsOut OUT>
PairsForm pairs_vb_form_of() {
  return {MT, NT, true, OUT, [](hipStream_t s, dim3 grid, const PairsArgs &a, int) {
            constexpr bool DENSE = OUT == PAIRS_DENSE;
            launch_pairs<k_pairs_tile_vb<MT, NT, DENSE>>(s, grid, DENSE ? 0 : PairsSel<MT>::BYTES, a);
          }};
}

PairsForm pairs_vb_form(const PairsRequest &rq) {
  if (rq.dense_form()) return pairs_vb_form_of<2, 2, PAIRS_DENSE>();
  if (rq.k <= 64) return pairs_vb_form_of<4, 1, PAIRS_SELECT>();
  if (rq.k <= 128) return pairs_vb_form_of<2, 2, PAIRS_SELECT>();
  return pairs_vb_form_of<1, 4, PAIRS_SELECT>();
}

// the six arrays of a variational model as a C-ABI call hands them over (host memory; V, V_var column-major (D, K))
struct PairsVbHost {
  int rank;
  double w0, w0_var, extra_var;
  const double *w, *w_var, *V, *V_var;
};

// the checks of the variational calls that need no device
void check_vb_model(const mfm_pairs *p, const PairsVbHost &h) {
  if (h.rank < 0) throw Error(MFM_ERR_INVALID, "rank must be non-negative");
  if (!(h.w0_var >= 0.0)) throw Error(MFM_ERR_INVALID, "w0_var must be non-negative");
  if (!(h.extra_var >= 0.0) || !std::isfinite(h.extra_var)) throw Error(MFM_ERR_INVALID, "extra_var must be finite and non-negative");
  if (p->D > 0 && (!h.w || !h.w_var || (h.rank > 0 && (!h.V || !h.V_var)))) throw Error(MFM_ERR_INVALID, "no posterior arrays");
}

void score_vb(mfm_pairs *p, const PairsVbHost &h, const PairsRequest &rq) {
  refuse_similarity_handle(p);
  check_vb_model(p, h);
  const bool is_dense = rq.dense_form();
  if (!is_dense && (rq.k < 1 || rq.k > PAIRS_MAX_K)) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  const PairsForm form = pairs_vb_form(rq);
  const int64_t U = p->U, I = p->I, D = p->D;
  if (U == 0 || (is_dense && I == 0)) return;
  hipStream_t s = p->stream;
  const PairsDims d = pairs_dims(p, PAIRS_VB_S, h.rank);
  const int K = d.K, KS = d.KS;

  // ---- the memory rule: Q and every block table resident, the query scratch bounded
  const double q_bytes = ((double)d.Ipad * d.S * KS + (double)d.Ipad * d.S) * sizeof(double);
  double t_bytes = 0.0;
  for (int side = 0; side < 2; side++)
    for (auto &b : p->blocks[side]) t_bytes += (double)b->M * (5 * KS + 3) * sizeof(double);
  if (exceeds_store_fraction(q_bytes + t_bytes))
    throw Error(MFM_ERR_RUNTIME, "pair scoring: the candidate side's embedding (" + std::to_string((int64_t)(q_bytes / 1048576.0)) +
                                     " MB) and the block tables (" + std::to_string((int64_t)(t_bytes / 1048576.0)) +
                                     " MB) exceed MFM_STORE_MAX_FRACTION of the free device memory; score fewer candidates or smaller blocks per call");

  // ---- the posterior on the device
  const size_t DK = (size_t)D * (size_t)K;
  DevBuf<double> model, d_w0;
  model.alloc(std::max<size_t>(2 * (size_t)D + 2 * DK, 1));
  if (D) {
    MFM_HIP_CHECK(hipMemcpy(model.p, h.w, (size_t)D * sizeof(double), hipMemcpyHostToDevice));
    MFM_HIP_CHECK(hipMemcpy(model.p + D, h.w_var, (size_t)D * sizeof(double), hipMemcpyHostToDevice));
    if (K) {
      MFM_HIP_CHECK(hipMemcpy(model.p + 2 * D, h.V, DK * sizeof(double), hipMemcpyHostToDevice));
      MFM_HIP_CHECK(hipMemcpy(model.p + 2 * D + DK, h.V_var, DK * sizeof(double), hipMemcpyHostToDevice));
    }
  }
  PairsVbModel pm;
  pm.w = model.p;
  pm.wv = model.p + D;
  pm.V = model.p + 2 * D;
  pm.Vv = model.p + 2 * D + DK;
  pm.D = D;
  pm.K = K;
  pm.KS = KS;
  pm.var0 = h.w0_var + h.extra_var;
  d_w0.upload(std::vector<double>{h.w0, 0.0, 0.0, 0.0, 0.0});

  // ---- the block tables of both sides, once per call
  std::vector<DevBuf<double>> tables[2];
  DevBuf<PairsVbBlockRef> d_blk[2];
  for (int side = 0; side < 2; side++) {
    std::vector<PairsVbBlockRef> refs;
    for (auto &b : p->blocks[side]) {
      const size_t M = (size_t)b->M;
      tables[side].emplace_back();
      DevBuf<double> &t = tables[side].back();
      t.alloc(std::max<size_t>(M * (size_t)(5 * KS + 3), 1));
      PairsVbBlockRef ref;
      ref.o2b = b->o2b.p;
      ref.T = t.p;
      ref.lin = t.p + M * (size_t)(5 * KS);
      ref.vv = ref.lin + M;
      ref.lv = ref.vv + M;
      ref.M = b->M;
      refs.push_back(ref);
      if (b->M > 0) {
        hipLaunchKernelGGL(k_pairs_vb_embed_block, dim3((unsigned)((b->M + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, b->ptr.p, b->idx.p,
                           b->val.p, b->M, b->off, pm, t.p, t.p + M * (size_t)(5 * KS), t.p + M * (size_t)(5 * KS + 1),
                           t.p + M * (size_t)(5 * KS + 2));
        MFM_HIP_CHECK(hipGetLastError());
      }
    }
    if (!refs.empty()) d_blk[side].upload(refs);
  }
  const auto embed = [&](int side, int64_t r0, int64_t R, int64_t Rpad, double *Pf, double *bias) {
    const dim3 grid((unsigned)((Rpad + PAIRS_WG - 1) / PAIRS_WG));
    const bool rel = !p->blocks[side].empty();
    const PairsVbBlockRef *blk = rel ? (const PairsVbBlockRef *)d_blk[side].p : nullptr;
    const int n_blk = (int)p->blocks[side].size();
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(PAIRS_WG), 0, s, side ? p->c_ptr.p : p->q_ptr.p, side ? p->c_idx.p : p->q_idx.p,
                         side ? p->c_val.p : p->q_val.p, r0, R, Rpad, pm, blk, n_blk, Pf, bias);
    };
    if (side == 1)
      rel ? launch(k_pairs_vb_embed<true, true>) : launch(k_pairs_vb_embed<false, true>);
    else
      rel ? launch(k_pairs_vb_embed<true, false>) : launch(k_pairs_vb_embed<false, false>);
  };

  Candidates cand;
  PairsArgs call = embed_candidates(p, d, rq, false, embed, cand);
  call.w0s = d_w0.p;
  walk_queries(p, form, call, rq, embed, [&](const PairsArgs &a, const int32_t *out_i, int64_t n, double *mean, double *sd) {
    hipLaunchKernelGGL(k_pairs_vb_at, dim3((unsigned)((n + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, a, out_i, n, mean, sd);
  });
}

static_assert(PAIRS_SIM_COSINE == MFM_PAIRS_SIM_COSINE && PAIRS_SIM_DOT == MFM_PAIRS_SIM_DOT, "the metrics as the header numbers them");

// ---- the requests of the entry points: each form's checks that need neither samples nor a device, once for its twins ------------
PairsRequest checked_scores(int mode, double *out) {
  if (!out) throw Error(MFM_ERR_INVALID, "no output array");
  PairsRequest rq{ASK_SCORES};
  rq.mode = mode;
  rq.dense = out;
  return rq;
}

PairsRequest checked_topk(int mode, int k, int64_t *idx, double *score) {
  if (!idx || !score) throw Error(MFM_ERR_INVALID, "no output array");
  PairsRequest rq{ASK_TOPK};
  rq.mode = mode;
  rq.k = k;
  rq.idx = idx;
  rq.value = score;
  return rq;
}

PairsRequest checked_moments(int mode, double *mean, double *sd) {
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  PairsRequest rq{ASK_MOMENTS};
  rq.mode = mode;
  rq.dense = mean;
  rq.sd = sd;
  return rq;
}

PairsRequest checked_ucb(int mode, int k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  if (!idx || !value || !mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  if (k < 1 || k > PAIRS_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  if (!std::isfinite(beta)) throw Error(MFM_ERR_INVALID, "beta must be a finite number");
  PairsRequest rq{ASK_UCB};
  rq.mode = mode;
  rq.k = k;
  rq.beta = beta;
  rq.idx = idx;
  rq.value = value;
  rq.mean = mean;
  rq.sd = sd;
  return rq;
}

void check_sim_metric(int metric) {
  if (metric != PAIRS_SIM_COSINE && metric != PAIRS_SIM_DOT)
    throw Error(MFM_ERR_INVALID, "bad similarity metric " + std::to_string(metric) + " (0: cosine, 1: dot)");
}

PairsRequest checked_sim_dense(const mfm_pairs *p, int metric, double *mean, double *sd) {
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  check_sim_metric(metric);
  if ((double)p->U * (double)p->I > 16777216.0)
    throw Error(MFM_ERR_INVALID, "the dense similarity call returns every pair: more than 2^24 pairs are refused, use mfm_pairs_topk_sim");
  PairsRequest rq{ASK_SIM};
  rq.metric = metric;
  rq.dense = mean;
  rq.sd = sd;
  return rq;
}

PairsRequest checked_topk_sim(int metric, int k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  PairsRequest rq = checked_ucb(0, k, beta, idx, value, mean, sd);
  check_sim_metric(metric);
  rq.ask = ASK_TOPK_SIM;
  rq.metric = metric;
  return rq;
}

PairsRequest checked_per_sample(PairsAsk ask, int mode, int k, const int32_t *row_sample, int n_top, int64_t *idx, double *value) {
  if (!idx || !value) throw Error(MFM_ERR_INVALID, "no output array");
  if (k < 1 || k > PAIRS_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  if (ask == ASK_VOTE && (n_top < 1 || n_top > PAIRS_VOTE_MAX_TOP)) throw Error(MFM_ERR_INVALID, "n_top must be in [1, 256]");
  PairsRequest rq{ask};
  rq.mode = mode;
  rq.k = k;
  rq.row_sample = row_sample;
  rq.n_top = n_top;
  rq.idx = idx;
  rq.value = value;
  return rq;
}

// (no output is needed while no target is stored)
PairsRequest checked_rank(const mfm_pairs *p, int mode, int64_t *rank_out, double *value_out) {
  if (p->has_targets && (!rank_out || !value_out)) throw Error(MFM_ERR_INVALID, "no output array");
  PairsRequest rq{ASK_RANK};
  rq.mode = mode;
  rq.target_rank = rank_out;
  rq.target_value = value_out;
  return rq;
}

PairsRequest checked_screened(int k, int64_t *idx, double *value, uint8_t *certified) {
  if (!idx || !value || !certified) throw Error(MFM_ERR_INVALID, "no output array");
  if (k < 1 || k > SCREEN_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 128]");
  PairsRequest rq{ASK_SCREENED};
  rq.k = k;
  rq.idx = idx;
  rq.value = value;
  rq.certified = certified;
  return rq;
}

PairsRequest checked_screen_dense(const mfm_pairs *p, double *r, double *bound) {
  if (!r || !bound) throw Error(MFM_ERR_INVALID, "no output array");
  if ((double)p->U * (double)p->I > 16777216.0)
    throw Error(MFM_ERR_INVALID, "the dense screening call returns every pair: more than 2^24 pairs are refused, use mfm_pairs_topk_screened");
  PairsRequest rq{ASK_SCREEN_DENSE};
  rq.dense = r;
  rq.bound = bound;
  return rq;
}

static_assert(DIV_MAX_POOL == MFM_PAIRS_DIVERSE_MAX_POOL, "the pool's limit as the header states it");

PairsRequest checked_diverse(int mode, int k, int pool, double lam, int64_t *idx, double *value, double *objective, double *redundancy) {
  if (!idx || !value || !objective || !redundancy) throw Error(MFM_ERR_INVALID, "no output array");
  if (pool < 1 || pool > DIV_MAX_POOL) throw Error(MFM_ERR_INVALID, "pool must be in [1, 128]");
  if (k < 1 || k > pool) throw Error(MFM_ERR_INVALID, "k must be in [1, pool]");
  if (!(lam >= 0.0 && lam <= 1.0)) throw Error(MFM_ERR_INVALID, "lam must be a finite number in [0, 1]");
  PairsRequest rq{ASK_DIVERSE};
  rq.mode = mode;
  rq.k = k;
  rq.pool = pool;
  rq.lam = lam;
  rq.idx = idx;
  rq.value = value;
  rq.objective = objective;
  rq.redundancy = redundancy;
  return rq;
}

// ---- where a call's samples come from: all that the _store and the host twin of a form differ in ---------------------------------
struct FromStore {
  mfm_store *st;
  int first, count;
  SampleView samples(const mfm_pairs *) const {
    if (!st) throw Error(MFM_ERR_INVALID, "no sample store");
    return samples_of_store(st, first, count);
  }
};

struct FromHost {
  int rank, n_samples;
  const double *w0s, *ws, *Vs;
  SampleView samples(const mfm_pairs *p) const { return samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs); }
};

// An entry point over samples: the form's checks (`checked`, one of the functions above), the refusal of a similarity handle for every
// form but its own, the samples, the call.
template <class From, class Checked>
int pairs_call(mfm_pairs *p, const From &from, Checked checked) {
  PAIRS_TRY(p)
  const PairsRequest rq = checked();
  if (!rq.sim()) refuse_similarity_handle(p);
  run_pairs(p, from.samples(p), rq);
  PAIRS_CATCH(p)
}

}  // namespace

extern "C" {

// both kinds of handle; `similarity`: no cross-side disjointness check (mfm_pairs_create_sim)
static int pairs_create(bool similarity, int device, int64_t D, int64_t U, const int64_t *q_indptr, const int32_t *q_indices,
                        const double *q_data, int64_t I, const int64_t *c_indptr, const int32_t *c_indices, const double *c_data,
                        mfm_pairs **out) {
  *out = nullptr;
  try {
    // (the arguments first: a machine without a GPU still learns that they are wrong)
    check_csr(U, D, q_indptr, q_indices, "X_query");
    check_csr(I, D, c_indptr, c_indices, "X_cand");
    if (I >= (int64_t)2147483647 - PAIRS_COL_ALIGN) throw Error(MFM_ERR_INVALID, "too many candidates");
    std::vector<uint8_t> seen((size_t)D, 0), seen_c((size_t)D, 0);
    for (int64_t q = 0; q < q_indptr[U]; q++) seen[(size_t)q_indices[q]] = 1;
    for (int64_t q = 0; q < c_indptr[I]; q++) {
      if (!similarity && seen[(size_t)c_indices[q]]) throw Error(MFM_ERR_INVALID, "X_query and X_cand share column " + std::to_string(c_indices[q]));
      seen_c[(size_t)c_indices[q]] = 1;
    }
    const int n = mfm_device_count();
    if (n <= 0)
      throw Error(MFM_ERR_DEVICE, "no HIP device is visible: libmyfm_hip.so has no CPU fallback (pair scoring runs on MI355X only)");
    if (device < 0 || device >= n) throw Error(MFM_ERR_INVALID, "device index out of range");
    std::unique_ptr<mfm_pairs> p(new mfm_pairs());
    p->device = device;
    p->similarity = similarity;
    p->use_device();
    MFM_HIP_CHECK(hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking));
    p->D = D;
    p->U = U;
    p->I = I;
    p->q_ptr.upload(q_indptr, (size_t)U + 1);
    p->q_idx.upload(q_indices, (size_t)q_indptr[U]);
    p->q_val.upload(q_data, (size_t)q_indptr[U]);
    p->c_ptr.upload(c_indptr, (size_t)I + 1);
    p->c_idx.upload(c_indices, (size_t)c_indptr[I]);
    p->c_val.upload(c_data, (size_t)c_indptr[I]);
    p->stored[0] = std::move(seen);
    p->stored[1] = std::move(seen_c);
    *out = p.release();
    return MFM_OK;
  } catch (const mfm::Error &ex) {
    g_pairs_error = ex.what();
    return ex.code;
  } catch (const std::exception &ex) {
    g_pairs_error = ex.what();
    return MFM_ERR_RUNTIME;
  }
}

int mfm_pairs_create(int device, int64_t D, int64_t U, const int64_t *q_indptr, const int32_t *q_indices, const double *q_data,
                     int64_t I, const int64_t *c_indptr, const int32_t *c_indices, const double *c_data, mfm_pairs **out) {
  return pairs_create(false, device, D, U, q_indptr, q_indices, q_data, I, c_indptr, c_indices, c_data, out);
}

int mfm_pairs_create_sim(int device, int64_t D, int64_t U, const int64_t *q_indptr, const int32_t *q_indices, const double *q_data,
                         int64_t I, const int64_t *c_indptr, const int32_t *c_indices, const double *c_data, mfm_pairs **out) {
  return pairs_create(true, device, D, U, q_indptr, q_indices, q_data, I, c_indptr, c_indices, c_data, out);
}

void mfm_pairs_destroy(mfm_pairs *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  delete p;
}

const char *mfm_pairs_last_error(const mfm_pairs *p) { return p ? p->err.c_str() : g_pairs_error.c_str(); }

int mfm_pairs_set_exclude(mfm_pairs *p, const int64_t *indptr, const int32_t *indices) {
  PAIRS_TRY(p)
  if (!indptr) {
    p->has_exclude = false;
    return MFM_OK;
  }
  check_csr(p->U, p->I, indptr, indices, "exclude");
  p->e_ptr_host.assign(indptr, indptr + p->U + 1);
  p->e_idx_host.assign(indices, indices + indptr[p->U]);
  p->has_exclude = indptr[p->U] > 0;
  try {
    check_targets_not_excluded(p);
  } catch (...) {
    p->has_exclude = false;
    throw;
  }
  p->e_ptr.upload(indptr, (size_t)p->U + 1);
  p->e_idx.upload(indices, (size_t)indptr[p->U]);
  PAIRS_CATCH(p)
}

int mfm_pairs_set_targets(mfm_pairs *p, const int64_t *indptr, const int32_t *indices) {
  PAIRS_TRY(p)
  if (!indptr) {
    p->has_targets = false;
    return MFM_OK;
  }
  check_csr(p->U, p->I, indptr, indices, "targets");
  for (int64_t u = 0; u < p->U; u++) {
    if (indptr[u + 1] - indptr[u] > PAIRS_RANK_MAX_T)
      throw Error(MFM_ERR_INVALID, "targets: query row " + std::to_string(u) + " has " + std::to_string(indptr[u + 1] - indptr[u]) +
                                       " targets, a call takes at most " + std::to_string(PAIRS_RANK_MAX_T) + " per row");
    for (int64_t q = indptr[u] + 1; q < indptr[u + 1]; q++)
      if (indices[q] <= indices[q - 1])
        throw Error(MFM_ERR_INVALID, "targets: the candidates of query row " + std::to_string(u) + " must be sorted and unique (candidate " +
                                         std::to_string(indices[q]) + " follows " + std::to_string(indices[q - 1]) + ")");
  }
  p->t_ptr_host.assign(indptr, indptr + p->U + 1);
  p->t_idx_host.assign(indices, indices + indptr[p->U]);
  p->has_targets = indptr[p->U] > 0;
  try {
    check_targets_not_excluded(p);
  } catch (...) {
    p->has_targets = false;
    throw;
  }
  p->t_ptr.upload(indptr, (size_t)p->U + 1);
  p->t_idx.upload(indices, (size_t)indptr[p->U]);
  PAIRS_CATCH(p)
}

int mfm_pairs_add_block(mfm_pairs *p, int32_t side, int64_t col_offset, int64_t width, int64_t block_rows, const int64_t *o2b,
                        const int64_t *indptr, const int32_t *indices, const double *data) {
  PAIRS_TRY(p)
  if (side != 0 && side != 1) throw Error(MFM_ERR_INVALID, "side must be 0 (query) or 1 (candidates), got " + std::to_string(side));
  const char *name = side == 0 ? "X_rel_query" : "X_rel_cand";
  const std::string what = std::string(name) + "[" + std::to_string(p->blocks[side].size()) + "]";
  if (col_offset < 0 || width < 0 || block_rows < 0) throw Error(MFM_ERR_INVALID, what + ": negative column offset or shape");
  if (col_offset > p->D || width > p->D - col_offset)
    throw Error(MFM_ERR_INVALID, what + ": columns [" + std::to_string(col_offset) + ", " + std::to_string(col_offset) + " + " +
                                     std::to_string(width) + ") exceed the feature size " + std::to_string(p->D));
  if (!o2b || !indptr) throw Error(MFM_ERR_INVALID, what + ": no index arrays");
  const int64_t R = side == 0 ? p->U : p->I;
  for (int64_t r = 0; r < R; r++)
    if (o2b[r] < 0 || o2b[r] >= block_rows)
      throw Error(MFM_ERR_INVALID, what + ": row " + std::to_string(r) + " maps to block row " + std::to_string(o2b[r]) + ", the block has " +
                                       std::to_string(block_rows));
  check_csr(block_rows, width, indptr, indices, what.c_str());
  const int64_t nnz = indptr[block_rows];
  // every stored column counts, referenced or not; nothing is marked before the whole block has passed
  for (int64_t q = 0; q < nnz; q++) {
    const size_t j = (size_t)(col_offset + indices[q]);
    if (!p->similarity && p->stored[1 - side][j]) throw Error(MFM_ERR_INVALID, "X_query and X_cand share column " + std::to_string(j));
  }
  {
    std::vector<uint8_t> own((size_t)width, 0);
    for (int64_t q = 0; q < nnz; q++) own[(size_t)indices[q]] = 1;
    for (int64_t j = 0; j < width; j++)
      if (own[(size_t)j] && p->stored[side][(size_t)(col_offset + j)])
        throw Error(MFM_ERR_INVALID, what + ": column " + std::to_string(col_offset + j) + " is already stored in this side");
  }
  std::unique_ptr<mfm_pairs::Block> b(new mfm_pairs::Block());
  b->off = col_offset;
  b->width = width;
  b->M = block_rows;
  b->o2b.upload(o2b, (size_t)R);
  b->ptr.upload(indptr, (size_t)block_rows + 1);
  b->idx.upload(indices, (size_t)nnz);
  b->val.upload(data, (size_t)nnz);
  for (int64_t q = 0; q < nnz; q++) p->stored[side][(size_t)(col_offset + indices[q])] = 1;
  p->blocks[side].push_back(std::move(b));
  PAIRS_CATCH(p)
}

int mfm_pairs_set_cutpoints(mfm_pairs *p, int32_t n_samples, int32_t n_cut, const double *cutpoints) {
  PAIRS_TRY(p)
  if (n_samples < 1 || n_cut < 1 || !cutpoints) throw Error(MFM_ERR_INVALID, "cutpoints: at least one sample and one cutpoint per sample");
  p->cut.assign(cutpoints, cutpoints + (size_t)n_samples * (size_t)n_cut);
  p->cut_S = n_samples;
  p->n_cut = n_cut;
  PAIRS_CATCH(p)
}

int mfm_pairs_set_scratch_bound(mfm_pairs *p, int64_t bytes) {
  PAIRS_TRY(p)
  if (bytes < 1) throw Error(MFM_ERR_INVALID, "the scratch bound must be positive");
  p->scratch_bound = bytes;
  PAIRS_CATCH(p)
}

int mfm_pairs_scores_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, double *out) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_scores(mode, out); });
}

int mfm_pairs_scores(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     int32_t mode, double *out) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_scores(mode, out); });
}

int mfm_pairs_topk_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int64_t *idx,
                         double *score) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_topk(mode, k, idx, score); });
}

int mfm_pairs_topk(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t mode, int32_t k, int64_t *idx, double *score) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_topk(mode, k, idx, score); });
}

int mfm_pairs_topk_screened_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t k, int64_t *idx, double *value,
                                  uint8_t *certified) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_screened(k, idx, value, certified); });
}

int mfm_pairs_topk_screened(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t k,
                            int64_t *idx, double *value, uint8_t *certified) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_screened(k, idx, value, certified); });
}

int mfm_pairs_topk_diverse_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int32_t pool, double lam,
                                 int64_t *idx, double *value, double *objective, double *redundancy) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_diverse(mode, k, pool, lam, idx, value, objective, redundancy); });
}

int mfm_pairs_topk_diverse(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t mode,
                           int32_t k, int32_t pool, double lam, int64_t *idx, double *value, double *objective, double *redundancy) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs},
                    [&] { return checked_diverse(mode, k, pool, lam, idx, value, objective, redundancy); });
}

int mfm_pairs_screen_scores_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, double *r, double *bound) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_screen_dense(p, r, bound); });
}

int mfm_pairs_screen_scores(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, double *r,
                            double *bound) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_screen_dense(p, r, bound); });
}

int mfm_pairs_moments_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, double *mean, double *sd) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_moments(mode, mean, sd); });
}

int mfm_pairs_moments(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                      int32_t mode, double *mean, double *sd) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_moments(mode, mean, sd); });
}

int mfm_pairs_topk_ucb_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *sd) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_ucb(mode, k, beta, idx, value, mean, sd); });
}

int mfm_pairs_topk_ucb(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t mode, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_ucb(mode, k, beta, idx, value, mean, sd); });
}

int mfm_pairs_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, double *mean, double *sd) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_sim_dense(p, metric, mean, sd); });
}

int mfm_pairs_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t metric,
                  double *mean, double *sd) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_sim_dense(p, metric, mean, sd); });
}

int mfm_pairs_topk_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *sd) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_topk_sim(metric, k, beta, idx, value, mean, sd); });
}

int mfm_pairs_topk_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t metric, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_topk_sim(metric, k, beta, idx, value, mean, sd); });
}

int mfm_pairs_topk_samples_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k,
                                 const int32_t *row_sample, int64_t *idx, double *value) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_per_sample(ASK_SAMPLES, mode, k, row_sample, 0, idx, value); });
}

int mfm_pairs_topk_samples(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t mode, int32_t k, const int32_t *row_sample, int64_t *idx, double *value) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_per_sample(ASK_SAMPLES, mode, k, row_sample, 0, idx, value); });
}

int mfm_pairs_topk_prob_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int32_t n_top,
                              int64_t *idx, double *prob) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_per_sample(ASK_VOTE, mode, k, nullptr, n_top, idx, prob); });
}

int mfm_pairs_topk_prob(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                        int32_t mode, int32_t k, int32_t n_top, int64_t *idx, double *prob) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_per_sample(ASK_VOTE, mode, k, nullptr, n_top, idx, prob); });
}

int mfm_pairs_rank_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int64_t *rank_out, double *value_out) {
  return pairs_call(p, FromStore{st, first, count}, [&] { return checked_rank(p, mode, rank_out, value_out); });
}

int mfm_pairs_rank(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t mode,
                   int64_t *rank_out, double *value_out) {
  return pairs_call(p, FromHost{rank, n_samples, w0s, ws, Vs}, [&] { return checked_rank(p, mode, rank_out, value_out); });
}

int mfm_pairs_moments_vb(mfm_pairs *p, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                         const double *V_var, double extra_var, double *mean, double *sd) {
  if (!p) {
    g_pairs_error = "mfm_pairs_moments_vb: no pair design";
    return MFM_ERR_INVALID;
  }
  PAIRS_TRY(p)
  const PairsRequest rq = checked_moments(0, mean, sd);
  score_vb(p, PairsVbHost{rank, w0, w0_var, extra_var, w, w_var, V, V_var}, rq);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_bound_vb(mfm_pairs *p, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                            const double *V_var, double extra_var, int32_t k, double beta, int64_t *idx, double *value, double *mean,
                            double *sd) {
  if (!p) {
    g_pairs_error = "mfm_pairs_topk_bound_vb: no pair design";
    return MFM_ERR_INVALID;
  }
  PAIRS_TRY(p)
  const PairsRequest rq = checked_ucb(0, k, beta, idx, value, mean, sd);
  score_vb(p, PairsVbHost{rank, w0, w0_var, extra_var, w, w_var, V, V_var}, rq);
  PAIRS_CATCH(p)
}

}  // extern "C"
