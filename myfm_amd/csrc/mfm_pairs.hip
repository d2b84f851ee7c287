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
// posterior instead of samples: run_pairs_vb at the end of this file, with the memory rule, the chunks and the stripes above.
#include "mfm_pairs.hpp"
#include "mfm_pairs_rank.hpp"
#include "mfm_pairs_samples.hpp"
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
PairsForm pairs_form(bool targets, bool spread, bool dense, int k, bool per_sample = false, bool sim = false) {
  if (sim) {
    if (dense) return pairs_sim_form_of<2, 2, PAIRS_DENSE>();
    if (k <= 64) return pairs_sim_form_of<4, 1, PAIRS_SELECT>();
    if (k <= 128) return pairs_sim_form_of<2, 2, PAIRS_SELECT>();
    return pairs_sim_form_of<1, 4, PAIRS_SELECT>();
  }
  if (targets) return pairs_form_of<4, 2, false, PAIRS_TARGETS>();
  if (per_sample) {
    if (k <= 64) return pairs_form_of<4, 2, false, PAIRS_SELECT_SAMPLE>();
    if (k <= 128) return pairs_form_of<2, 4, false, PAIRS_SELECT_SAMPLE>();
    return pairs_form_of<1, 8, false, PAIRS_SELECT_SAMPLE>();
  }
  if (!spread) {
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

// what a moments call adds to a mean call: rank by mean + beta * std, and return mean and std ((U, I) each with `dense`, which
// then holds the mean; (U, k) each with the top k)
struct PairsMoments {
  double beta = 0.0;
  double *mean = nullptr, *sd = nullptr;
};

// the outputs of a rank call, one entry per stored target in CSR order
struct PairsRank {
  int64_t *rank = nullptr;
  double *value = nullptr;
};

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
// what a per-sample call asks for
struct PairsPerSample {
  const int32_t *row_sample = nullptr;  // [U]: only the list of row u's own sample, outputs [U][k]; null: every sample's, [S][U][k]
  int n_top = 0;                        // > 0: the vote over every sample's list; idx / value are [U][n_top] indices / probabilities
  int64_t *idx = nullptr;
  double *value = nullptr;
};

static_assert(PAIRS_VOTE_MAX == MFM_PAIRS_VOTE_MAX && PAIRS_VOTE_MAX >= 95 * PAIRS_MAX_K, "the vote's limit as the header states it");

// the checks that need the sample count (before any launch)
void check_per_sample(const PairsPerSample &ps, int S, int k, int64_t U) {
  if (ps.row_sample)
    for (int64_t u = 0; u < U; u++)
      if (ps.row_sample[u] < 0 || ps.row_sample[u] >= S)
        throw Error(MFM_ERR_INVALID, "row_sample: query row " + std::to_string(u) + " asks for sample " + std::to_string(ps.row_sample[u]) +
                                         ", the call has " + std::to_string(S));
  if (ps.n_top > 0 && (int64_t)S * k > PAIRS_VOTE_MAX)
    throw Error(MFM_ERR_INVALID, "the vote takes at most " + std::to_string(PAIRS_VOTE_MAX) + " list entries per query row (samples * k), the call has " +
                                     std::to_string((int64_t)S * k));
}

// The queries in chunks, each chunk's plan in slices (the candidate side is resident: `call`).
// Chunk: its per-row scratch -- P and the biases (all samples, or the row's own with the two maps), the exclusion bitmask, the
// votes and the voted result -- stays under HALF the scratch bound (never less than one 64-row tile). Slice: consecutive plan
// entries whose stripe lists and merged lists fit what the chunk's scratch leaves of the bound (never less than one entry). The
// stripes are chosen per chunk from its entry count, as the other forms choose them from their row tiles. Every list is merged
// under the selection's total order and lands at a place that its (sample, row) alone decides, so neither the bound nor the
// stripes nor the slices change a bit of the results.
template <class Embed>
void walk_samples(mfm_pairs *p, const PairsForm &form, const PairsArgs &call, int mode, const PairsPerSample &ps, Embed embed) {
  hipStream_t s = p->stream;
  const int S = call.S, k = call.k, KS = call.KS4 * 4, rows = form.rows();
  const int64_t U = p->U, I = call.I, W = call.W;
  const bool own = ps.row_sample != nullptr, vote = ps.n_top > 0, masked = p->has_exclude;
  const double per_row = (own ? (double)KS * 8 + 16 : (double)S * KS * 8 + (double)S * 8) + (masked ? (double)W * 4 : 0.0) +
                         (vote ? (double)S * k * 4 + (double)ps.n_top * 12 : 0.0);
  int64_t chunk = (int64_t)std::min<double>((double)(p->scratch_bound / 2) / per_row, 1e12);
  chunk = std::max<int64_t>(chunk / PAIRS_ROW_ALIGN * PAIRS_ROW_ALIGN, PAIRS_ROW_ALIGN);
  chunk = std::min<int64_t>(chunk, round_up(U, PAIRS_ROW_ALIGN));
  const int64_t steps_total = (std::max<int64_t>(I, 1) + form.step() - 1) / form.step();
  int n_sort = 2;  // the vote's sort length: the power of two at or above S * k
  while (vote && n_sort < S * k) n_sort <<= 1;

  DevBuf<double> Pf, Ab, list_v, out_v, res_p;
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
      for (int64_t u = 0; u < Uc; u++) fill[(size_t)ps.row_sample[u0 + u]]++;
      Ppad = 0;
      for (int g = 0; g < S; g++) {
        const int64_t n_g = fill[(size_t)g];
        fill[(size_t)g] = Ppad;  // (from here on: where the group's next row goes)
        for (int64_t t = 0; t < n_g; t += rows) plan.push_back({Ppad + t, 0, g, (int32_t)std::min<int64_t>(rows, n_g - t)});
        Ppad += round_up(n_g, rows);
      }
      row_of.assign((size_t)Ppad, -1);
      map_s.assign((size_t)Ppad, 0);
      for (int64_t u = 0; u < Uc; u++) row_of[(size_t)fill[(size_t)ps.row_sample[u0 + u]]++] = (int32_t)u;
      for (const PairsPlanEntry &e : plan)
        for (int r = 0; r < rows; r++) map_s[(size_t)e.row0 + r] = e.s;
    } else {
      for (int g = 0; g < S; g++)
        for (int64_t t = 0; t < Uc; t += rows) plan.push_back({t, 0, g, (int32_t)std::min<int64_t>(rows, Uc - t)});
    }
    const int64_t n_e = (int64_t)plan.size();
    if (n_e == 0) continue;
    // stripes: enough workgroups to fill the device twice, at most PAIRS_MAX_STRIPES lists to merge
    int64_t n_stripes = std::max<int64_t>(1, std::min<int64_t>({(512 + n_e - 1) / n_e, steps_total, (int64_t)PAIRS_MAX_STRIPES}));
    const int64_t stripe_steps = (steps_total + n_stripes - 1) / n_stripes;
    n_stripes = (steps_total + stripe_steps - 1) / stripe_steps;
    // slices: what the chunk's own scratch leaves of the bound, in entries
    const double fixed = (own ? (double)Ppad * (KS * 8 + 16) : (double)Upad * S * (KS + 1) * 8) + (masked ? (double)Uc * W * 4 : 0.0) +
                         (vote ? (double)Uc * ((double)S * k * 4 + (double)ps.n_top * 12) : 0.0);
    const double per_entry = (double)(n_stripes + 1) * rows * k * 12 + sizeof(PairsPlanEntry);
    const int64_t slice = std::max<int64_t>(1, (int64_t)std::min<double>(((double)p->scratch_bound - fixed) / per_entry, (double)n_e));
    for (int64_t e = 0; e < n_e; e++) plan[(size_t)e].out = (e % slice) * rows;
    d_plan.upload(plan);
    if (own) {
      d_row_of.upload(row_of);
      d_map_s.upload(map_s);
    }
    // ---- P, the mask
    ensure(Pf, (size_t)(Ppad * (own ? (int64_t)KS : (int64_t)S * KS)));
    ensure(Ab, (size_t)(own ? Ppad : Upad * S));
    embed(0, p->q_ptr.p, p->q_idx.p, p->q_val.p, u0, Uc, Ppad, Pf.p, Ab.p, own ? d_row_of.p : nullptr, own ? d_map_s.p : nullptr);
    MFM_HIP_CHECK(hipGetLastError());
    const bool use_mask = masked && p->e_ptr_host[u0 + Uc] > p->e_ptr_host[u0];
    if (use_mask) {
      ensure(mask, (size_t)(Uc * W));
      MFM_HIP_CHECK(hipMemsetAsync(mask.p, 0, (size_t)(Uc * W) * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_pairs_mask, dim3((unsigned)((Uc + 3) / 4)), dim3(PAIRS_WG), 0, s, p->e_ptr.p, p->e_idx.p, u0, Uc, W, mask.p);
    }
    PairsArgs a = call;
    a.Pf = Pf.p;
    a.p_stride = own ? (int64_t)call.KS4 : call.NK;
    a.Ab = Ab.p;
    a.Upad = Upad;
    a.Uc = Uc;
    a.stripe_len = stripe_steps * form.step();
    a.mask = use_mask ? mask.p : nullptr;
    a.u0 = u0;
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
        form.launch(s, dim3((unsigned)E, (unsigned)n_stripes), a, mode);
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
            ps.idx[o + j] = h_idx[l + j];
            ps.value[o + j] = h_val[l + j];
          }
        }
      }
    }
    if (vote) {
      ensure(res_i, (size_t)(Uc * ps.n_top));
      ensure(res_p, (size_t)(Uc * ps.n_top));
      const size_t lds = (size_t)n_sort * sizeof(int);
      static DeviceOnce raised;
      if (lds > 48 * 1024 && raised.need()) {
        MFM_HIP_CHECK(hipFuncSetAttribute((const void *)k_pairs_vote, hipFuncAttributeMaxDynamicSharedMemorySize, PAIRS_VOTE_MAX * (int)sizeof(int)));
        raised.mark();
      }
      hipLaunchKernelGGL(k_pairs_vote, dim3((unsigned)Uc), dim3(PAIRS_WG), lds, s, votes.p, S * k, n_sort, S, ps.n_top, res_i.p, res_p.p);
      MFM_HIP_CHECK(hipGetLastError());
      h_idx.resize((size_t)(Uc * ps.n_top));
      MFM_HIP_CHECK(hipMemcpyAsync(ps.value + (size_t)u0 * ps.n_top, res_p.p, (size_t)(Uc * ps.n_top) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), res_i.p, (size_t)(Uc * ps.n_top) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      for (int64_t e = 0; e < Uc * ps.n_top; e++) ps.idx[u0 * ps.n_top + e] = h_idx[(size_t)e];
    }
    MFM_HIP_CHECK(hipStreamSynchronize(s));
  }
}

// The whole call over the samples of `v` (mfm_samples.hpp). dense != nullptr: (U, I) scores; else the top k. mo != nullptr: the
// moments form. rk != nullptr: the rank form (neither dense nor k). ps != nullptr: the per-sample selecting form (k, its own outputs).
// sim >= 0: the similarity forms under that metric (PAIRS_SIM_*; with mo, mode 0): the embeddings carry the normalisation in the
// bias slot and no bias is summed; everything else -- the memory rule, the chunks, the stripes, the merge -- is the moments call's.
void run_pairs(mfm_pairs *p, const SampleView &v, int mode, int k, int64_t *idx, double *score, double *dense,
               const PairsMoments *mo = nullptr, const PairsRank *rk = nullptr, const PairsPerSample *ps = nullptr, int sim = -1) {
  const int S = v.count(), rank = v.K;
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
  const bool is_dense = dense != nullptr;
  if (!is_dense && !rk && (k < 1 || k > PAIRS_MAX_K)) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  // the form of the call, decided here once: the scratch per query row, the stripes, the grid and the launch all read it
  const PairsForm form = pairs_form(rk != nullptr, mo != nullptr, is_dense, k, ps != nullptr, sim >= 0);
  const int64_t U = p->U, I = p->I, D = p->D;
  if (ps) check_per_sample(*ps, S, k, U);
  if (U == 0 || (is_dense && I == 0)) return;
  if (rk && (I == 0 || !p->has_targets)) return;
  hipStream_t s = p->stream;
  const int K = rank, KS = (K + 3) & ~3, KS4 = KS / 4;
  const int64_t NK = (int64_t)S * KS4;
  const int64_t Ipad = round_up(std::max<int64_t>(I, 1), PAIRS_COL_ALIGN);

  // ---- the memory rule: Q and every block table resident, the query scratch bounded
  const double q_bytes = ((double)Ipad * S * KS + (double)Ipad * (S + 1)) * sizeof(double);
  double t_bytes[2] = {0.0, 0.0};
  for (int side = 0; side < 2; side++)
    for (auto &b : p->blocks[side]) t_bytes[side] += (double)b->M * S * (KS + 2) * sizeof(double);
  {
    size_t free_b = 0, total_b = 0;
    const double frac = env_double("MFM_STORE_MAX_FRACTION", 0.5);
    const double all_bytes = q_bytes + t_bytes[0] + t_bytes[1];
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && all_bytes > frac * (double)free_b) {
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
  }
  const int64_t W = (I + 31) / 32;
  const int64_t steps_total = (std::max<int64_t>(I, 1) + form.step() - 1) / form.step();
  const double per_row = (double)S * KS * 8 + (double)(S + 1) * 8 + (p->has_exclude && form.out != PAIRS_DENSE ? (double)W * 4 : 0.0) +
                         (form.out == PAIRS_DENSE     ? (double)I * 8
                          : form.out == PAIRS_TARGETS ? (double)PAIRS_RANK_MAX_T * 12  // (the targets' values and ranks)
                                                      : (double)(PAIRS_MAX_STRIPES + 1) * k * 12) +
                         // (the second dense output / mean and std of the lists)
                         (!form.spread ? 0.0 : form.out == PAIRS_DENSE ? (double)I * 8 : (double)k * 16);
  int64_t chunk = (int64_t)std::min<double>((double)p->scratch_bound / per_row, 1e12);
  chunk = std::max<int64_t>(chunk / PAIRS_ROW_ALIGN * PAIRS_ROW_ALIGN, PAIRS_ROW_ALIGN);
  chunk = std::min<int64_t>(chunk, round_up(U, PAIRS_ROW_ALIGN));

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
  // a side with blocks gathers from its tables, one without takes the instantiation that reads no block argument
  // (map_row / map_s: the row -> sample plan's flavour, one launch row per row of P under its own sample)
  const auto embed = [&](int side, const int64_t *ptr, const int32_t *idx, const double *val, int64_t r0, int64_t R, int64_t Rpad, double *Pf,
                         double *bias, const int32_t *map_row, const int32_t *map_s) {
    const dim3 grid((unsigned)((Rpad + PAIRS_WG - 1) / PAIRS_WG), map_row ? 1u : (unsigned)S);
    const bool rel = !p->blocks[side].empty();
    const PairsBlockRef *blk = rel ? (const PairsBlockRef *)d_blk[side].p : nullptr;
    const int n_blk = (int)p->blocks[side].size();
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(PAIRS_WG), 0, s, ptr, idx, val, r0, R, Rpad, (const double *const *)d_wv.p, D, K, KS, S, blk,
                         n_blk, Pf, bias, map_row, map_s);
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

  // ---- candidate side, once
  DevBuf<double> Qf, Bb, Bsum;
  Qf.alloc((size_t)std::max<int64_t>(Ipad * NK * 4, 1));
  Bb.alloc((size_t)Ipad * S);
  if (sim < 0) Bsum.alloc((size_t)Ipad);  // (the similarity finish reads the per-sample slots alone: no sums, Asum / Bsum stay null)
  embed(1, p->c_ptr.p, p->c_idx.p, p->c_val.p, (int64_t)0, I, Ipad, Qf.p, Bb.p, nullptr, nullptr);
  if (sim < 0) hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)(Ipad / PAIRS_WG)), dim3(PAIRS_WG), 0, s, Bb.p, S, Ipad, Bsum.p);
  MFM_HIP_CHECK(hipGetLastError());

  // ---- what every launch of the call reads; a chunk adds its own
  PairsArgs call;
  call.Pf = nullptr;
  call.Qf = Qf.p;
  call.NK = NK;
  call.p_stride = NK;
  call.q_stride = NK;
  call.KS4 = KS4;
  call.S = S;
  call.Ab = nullptr;
  call.Asum = nullptr;
  call.Bb = Bb.p;
  call.Bsum = Bsum.p;
  call.w0s = d_w0.p;
  call.w0sum = w0sum;
  call.cut = mode == 2 ? d_cut.p : nullptr;
  call.n_cut = mode == 2 ? p->n_cut : 0;
  call.beta = mo ? mo->beta : 0.0;
  call.Upad = 0;
  call.Ipad = Ipad;
  call.Uc = 0;
  call.I = I;
  call.stripe_len = 0;
  call.dense = nullptr;
  call.dense_std = nullptr;
  call.mask = nullptr;
  call.W = W;
  call.k = k;
  call.list_v = nullptr;
  call.list_i = nullptr;
  call.tptr = nullptr;
  call.tidx = nullptr;
  call.tval = nullptr;
  call.trank = nullptr;
  call.u0 = 0;
  call.tbase = 0;
  call.plan = nullptr;
  call.row_of = nullptr;
  call.list_rows = 0;
  if (ps) {
    walk_samples(p, form, call, mode, *ps, embed);
    return;
  }

  // ---- queries, chunk by chunk
  DevBuf<double> Pf, Ab, Asum, list_v, out_v, d_dense, d_dense_std, out_m, out_s;
  DevBuf<int32_t> list_i, out_i;
  DevBuf<uint32_t> mask;
  DevBuf<int32_t> t_rank;
  DevBuf<double> t_val;
  std::vector<int32_t> h_idx;
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    const int64_t tbase = rk ? p->t_ptr_host[u0] : 0, n_t = rk ? p->t_ptr_host[u0 + Uc] - tbase : 0;
    if (rk && n_t == 0) continue;
    ensure(Pf, (size_t)(Upad * NK * 4));
    ensure(Ab, (size_t)(Upad * S));
    if (sim < 0) ensure(Asum, (size_t)Upad);
    embed(0, p->q_ptr.p, p->q_idx.p, p->q_val.p, u0, Uc, Upad, Pf.p, Ab.p, nullptr, nullptr);
    if (sim < 0)
      hipLaunchKernelGGL(k_pairs_bias_sum, dim3((unsigned)((Upad + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, Ab.p, S, Upad,
                         Asum.p);
    const bool use_mask = !is_dense && p->has_exclude && p->e_ptr_host[u0 + Uc] > p->e_ptr_host[u0];
    if (use_mask) {
      ensure(mask, (size_t)(Uc * W));
      MFM_HIP_CHECK(hipMemsetAsync(mask.p, 0, (size_t)(Uc * W) * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_pairs_mask, dim3((unsigned)((Uc + 3) / 4)), dim3(PAIRS_WG), 0, s, p->e_ptr.p, p->e_idx.p, u0, Uc, W, mask.p);
    }
    // stripes: enough workgroups to fill the device twice, at most PAIRS_MAX_STRIPES lists to merge
    const int64_t n_qt = Upad / form.rows();
    int64_t n_stripes = std::max<int64_t>(1, std::min<int64_t>({(512 + n_qt - 1) / n_qt, steps_total, (int64_t)PAIRS_MAX_STRIPES}));
    const int64_t stripe_steps = (steps_total + n_stripes - 1) / n_stripes;
    n_stripes = (steps_total + stripe_steps - 1) / stripe_steps;
    const dim3 grid((unsigned)n_qt, (unsigned)n_stripes);
    PairsArgs a = call;
    a.Pf = Pf.p;
    a.Ab = Ab.p;
    a.Asum = Asum.p;
    a.Upad = Upad;
    a.Uc = Uc;
    a.stripe_len = stripe_steps * form.step();
    a.mask = use_mask ? mask.p : nullptr;
    a.list_rows = Upad;
    a.u0 = u0;
    a.tbase = tbase;
    if (rk) {
      ensure(t_val, (size_t)n_t);
      ensure(t_rank, (size_t)n_t);
      a.tptr = p->t_ptr.p;
      a.tidx = p->t_idx.p;
      a.tval = t_val.p;
      a.trank = t_rank.p;
      MFM_HIP_CHECK(hipMemsetAsync(t_rank.p, 0, (size_t)n_t * sizeof(int32_t), s));
      form.launch(s, grid, a, mode);
      MFM_HIP_CHECK(hipGetLastError());
      h_idx.resize((size_t)n_t);
      MFM_HIP_CHECK(hipMemcpyAsync(rk->value + tbase, t_val.p, (size_t)n_t * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), t_rank.p, (size_t)n_t * sizeof(int32_t), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      for (int64_t e = 0; e < n_t; e++) rk->rank[tbase + e] = h_idx[(size_t)e];
      continue;
    }
    if (is_dense) {
      ensure(d_dense, (size_t)(Uc * I));
      a.dense = d_dense.p;
      if (mo) {
        ensure(d_dense_std, (size_t)(Uc * I));
        a.dense_std = d_dense_std.p;
      }
      form.launch(s, grid, a, mode);
      MFM_HIP_CHECK(hipGetLastError());
      if (mo)
        MFM_HIP_CHECK(
            hipMemcpyAsync(mo->sd + (size_t)u0 * I, d_dense_std.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(dense + (size_t)u0 * I, d_dense.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
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
      form.launch(s, grid, a, mode);
      MFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)Uc), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, Upad, k,
                       out_v.p, out_i.p);
    MFM_HIP_CHECK(hipGetLastError());
    if (mo) {
      ensure(out_m, (size_t)(Uc * k));
      ensure(out_s, (size_t)(Uc * k));
      launch_moments_at(s, a, mode, form.sim, out_i.p, Uc * k, out_m.p, out_s.p);
      MFM_HIP_CHECK(hipGetLastError());
      MFM_HIP_CHECK(hipMemcpyAsync(mo->mean + (size_t)u0 * k, out_m.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(mo->sd + (size_t)u0 * k, out_s.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    h_idx.resize((size_t)(Uc * k));
    MFM_HIP_CHECK(hipMemcpyAsync(score + (size_t)u0 * k, out_v.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), out_i.p, (size_t)(Uc * k) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t e = 0; e < Uc * k; e++) idx[u0 * k + e] = h_idx[(size_t)e];
  }
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

// A similarity handle's sides may share columns: the score's split into per-side terms and one contraction is wrong there, so every
// scoring form is refused on it, before the samples are looked at.
void refuse_similarity_handle(const mfm_pairs *p) {
  if (p->similarity)
    throw Error(MFM_ERR_INVALID, "this is a similarity handle (mfm_pairs_create_sim): its sides may share columns, which the pair score's "
                                 "decomposition does not allow; it serves mfm_pairs_sim* and mfm_pairs_topk_sim* only");
}

void run_pairs_store(mfm_pairs *p, mfm_store *st, int first, int count, int mode, int k, int64_t *idx, double *score, double *dense,
                     const PairsMoments *mo = nullptr, const PairsRank *rk = nullptr, const PairsPerSample *ps = nullptr, int sim = -1) {
  if (sim < 0) refuse_similarity_handle(p);
  if (!st) throw Error(MFM_ERR_INVALID, "no sample store");
  run_pairs(p, samples_of_store(st, first, count), mode, k, idx, score, dense, mo, rk, ps, sim);
}

void run_pairs_host(mfm_pairs *p, int rank, int n_samples, const double *w0s, const double *ws, const double *Vs, int mode, int k,
                    int64_t *idx, double *score, double *dense, const PairsMoments *mo = nullptr, const PairsRank *rk = nullptr,
                    const PairsPerSample *ps = nullptr, int sim = -1) {
  if (sim < 0) refuse_similarity_handle(p);
  run_pairs(p, samples_of_host(p->device, p->D, rank, n_samples, w0s, ws, Vs), mode, k, idx, score, dense, mo, rk, ps, sim);
}

static_assert(PAIRS_SIM_COSINE == MFM_PAIRS_SIM_COSINE && PAIRS_SIM_DOT == MFM_PAIRS_SIM_DOT, "the metrics as the header numbers them");

// the checks of the similarity calls that need neither samples nor a device
void check_sim_metric(int metric) {
  if (metric != PAIRS_SIM_COSINE && metric != PAIRS_SIM_DOT)
    throw Error(MFM_ERR_INVALID, "bad similarity metric " + std::to_string(metric) + " (0: cosine, 1: dot)");
}

PairsMoments checked_sim_dense(const mfm_pairs *p, int metric, double *mean, double *sd) {
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  check_sim_metric(metric);
  if ((double)p->U * (double)p->I > 16777216.0)
    throw Error(MFM_ERR_INVALID, "the dense similarity call returns every pair: more than 2^24 pairs are refused, use mfm_pairs_topk_sim");
  PairsMoments mo;
  mo.sd = sd;
  return mo;
}

// the checks of the per-sample calls that need neither samples nor a device
PairsPerSample checked_per_sample(int k, const int32_t *row_sample, int n_top, bool vote, int64_t *idx, double *value) {
  if (!idx || !value) throw Error(MFM_ERR_INVALID, "no output array");
  if (k < 1 || k > PAIRS_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  if (vote && (n_top < 1 || n_top > PAIRS_VOTE_MAX_TOP)) throw Error(MFM_ERR_INVALID, "n_top must be in [1, 256]");
  PairsPerSample ps;
  ps.row_sample = row_sample;
  ps.n_top = vote ? n_top : 0;
  ps.idx = idx;
  ps.value = value;
  return ps;
}

// the outputs of a rank call: none is needed while no target is stored
PairsRank checked_rank(const mfm_pairs *p, int64_t *rank_out, double *value_out) {
  if (p->has_targets && (!rank_out || !value_out)) throw Error(MFM_ERR_INVALID, "no output array");
  PairsRank rk;
  rk.rank = rank_out;
  rk.value = value_out;
  return rk;
}

// the checks of the ranked moments calls that need neither samples nor a device
PairsMoments checked_ucb(int k, double beta, const int64_t *idx, const double *value, double *mean, double *sd) {
  if (!idx || !value || !mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  if (k < 1 || k > PAIRS_MAX_K) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  if (!std::isfinite(beta)) throw Error(MFM_ERR_INVALID, "beta must be a finite number");
  PairsMoments mo;
  mo.beta = beta;
  mo.mean = mean;
  mo.sd = sd;
  return mo;
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
  PAIRS_TRY(p)
  if (!out) throw Error(MFM_ERR_INVALID, "no output array");
  run_pairs_store(p, st, first, count, mode, 0, nullptr, nullptr, out);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int64_t *idx,
                         double *score) {
  PAIRS_TRY(p)
  if (!idx || !score) throw Error(MFM_ERR_INVALID, "no output array");
  run_pairs_store(p, st, first, count, mode, k, idx, score, nullptr);
  PAIRS_CATCH(p)
}

int mfm_pairs_scores(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     int32_t mode, double *out) {
  PAIRS_TRY(p)
  if (!out) throw Error(MFM_ERR_INVALID, "no output array");
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, 0, nullptr, nullptr, out);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t mode, int32_t k, int64_t *idx, double *score) {
  PAIRS_TRY(p)
  if (!idx || !score) throw Error(MFM_ERR_INVALID, "no output array");
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, k, idx, score, nullptr);
  PAIRS_CATCH(p)
}

int mfm_pairs_moments_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, double *mean, double *sd) {
  PAIRS_TRY(p)
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  PairsMoments mo;
  mo.sd = sd;
  run_pairs_store(p, st, first, count, mode, 0, nullptr, nullptr, mean, &mo);
  PAIRS_CATCH(p)
}

int mfm_pairs_moments(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                      int32_t mode, double *mean, double *sd) {
  PAIRS_TRY(p)
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  PairsMoments mo;
  mo.sd = sd;
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, 0, nullptr, nullptr, mean, &mo);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_ucb_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_ucb(k, beta, idx, value, mean, sd);
  run_pairs_store(p, st, first, count, mode, k, idx, value, nullptr, &mo);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_ucb(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t mode, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_ucb(k, beta, idx, value, mean, sd);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, k, idx, value, nullptr, &mo);
  PAIRS_CATCH(p)
}

int mfm_pairs_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_sim_dense(p, metric, mean, sd);
  run_pairs_store(p, st, first, count, 0, 0, nullptr, nullptr, mean, &mo, nullptr, nullptr, metric);
  PAIRS_CATCH(p)
}

int mfm_pairs_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t metric,
                  double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_sim_dense(p, metric, mean, sd);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, 0, 0, nullptr, nullptr, mean, &mo, nullptr, nullptr, metric);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_ucb(k, beta, idx, value, mean, sd);
  check_sim_metric(metric);
  run_pairs_store(p, st, first, count, 0, k, idx, value, nullptr, &mo, nullptr, nullptr, metric);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t metric, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *sd) {
  PAIRS_TRY(p)
  const PairsMoments mo = checked_ucb(k, beta, idx, value, mean, sd);
  check_sim_metric(metric);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, 0, k, idx, value, nullptr, &mo, nullptr, nullptr, metric);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_samples_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k,
                                 const int32_t *row_sample, int64_t *idx, double *value) {
  PAIRS_TRY(p)
  const PairsPerSample ps = checked_per_sample(k, row_sample, 0, false, idx, value);
  run_pairs_store(p, st, first, count, mode, k, nullptr, nullptr, nullptr, nullptr, nullptr, &ps);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_samples(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t mode, int32_t k, const int32_t *row_sample, int64_t *idx, double *value) {
  PAIRS_TRY(p)
  const PairsPerSample ps = checked_per_sample(k, row_sample, 0, false, idx, value);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, k, nullptr, nullptr, nullptr, nullptr, nullptr, &ps);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_prob_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int32_t n_top,
                              int64_t *idx, double *prob) {
  PAIRS_TRY(p)
  const PairsPerSample ps = checked_per_sample(k, nullptr, n_top, true, idx, prob);
  run_pairs_store(p, st, first, count, mode, k, nullptr, nullptr, nullptr, nullptr, nullptr, &ps);
  PAIRS_CATCH(p)
}

int mfm_pairs_topk_prob(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                        int32_t mode, int32_t k, int32_t n_top, int64_t *idx, double *prob) {
  PAIRS_TRY(p)
  const PairsPerSample ps = checked_per_sample(k, nullptr, n_top, true, idx, prob);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, k, nullptr, nullptr, nullptr, nullptr, nullptr, &ps);
  PAIRS_CATCH(p)
}

int mfm_pairs_rank_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int64_t *rank_out, double *value_out) {
  PAIRS_TRY(p)
  const PairsRank rk = checked_rank(p, rank_out, value_out);
  run_pairs_store(p, st, first, count, mode, 0, nullptr, nullptr, nullptr, nullptr, &rk);
  PAIRS_CATCH(p)
}

int mfm_pairs_rank(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t mode,
                   int64_t *rank_out, double *value_out) {
  PAIRS_TRY(p)
  const PairsRank rk = checked_rank(p, rank_out, value_out);
  run_pairs_host(p, rank, n_samples, w0s, ws, Vs, mode, 0, nullptr, nullptr, nullptr, nullptr, &rk);
  PAIRS_CATCH(p)
}

}  // extern "C"

// ---- the variational forms (mfm_pairs_vb.hpp) ----------------------------------------------------------------------
// Analytic mean and standard deviation of the score of every pair under the posterior N(w0, w0_var), N(w, w_var), N(V, V_var): five
// pseudo-samples of width KS through the per-sample contraction. The handle's sides, blocks, exclusions, scratch bound and query
// chunking are run_pairs', with S = 5 in every formula; the tile shapes are the moments forms' (MT NT = 4).
namespace {

struct PairsVbForm {
  int MT, NT;
  void (*launch)(hipStream_t, dim3, const PairsArgs &);
  int rows() const { return 16 * MT; }
  int step() const { return 64 * NT; }
};

template <int MT, int NT, bool DENSE>
void launch_vb_form(hipStream_t s, dim3 grid, const PairsArgs &a) {
  launch_pairs<k_pairs_tile_vb<MT, NT, DENSE>>(s, grid, DENSE ? 0 : PairsSel<MT>::BYTES, a);
}

PairsVbForm pairs_vb_form(bool dense, int k) {
  if (dense) return {2, 2, &launch_vb_form<2, 2, true>};
  if (k <= 64) return {4, 1, &launch_vb_form<4, 1, false>};
  if (k <= 128) return {2, 2, &launch_vb_form<2, 2, false>};
  return {1, 4, &launch_vb_form<1, 4, false>};
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

// dense != nullptr: (U, I) mean into dense and std into mo.sd; else the top k by mean + mo.beta * std (idx, score, mo.mean, mo.sd)
void run_pairs_vb(mfm_pairs *p, const PairsVbHost &h, int k, int64_t *idx, double *score, double *dense, const PairsMoments &mo) {
  refuse_similarity_handle(p);
  check_vb_model(p, h);
  const bool is_dense = dense != nullptr;
  if (!is_dense && (k < 1 || k > PAIRS_MAX_K)) throw Error(MFM_ERR_INVALID, "k must be in [1, 256]");
  const PairsVbForm form = pairs_vb_form(is_dense, k);
  const int64_t U = p->U, I = p->I, D = p->D;
  if (U == 0 || (is_dense && I == 0)) return;
  hipStream_t s = p->stream;
  const int S = PAIRS_VB_S, K = h.rank, KS = (K + 3) & ~3, KS4 = KS / 4;
  const int64_t NK = (int64_t)S * KS4;
  const int64_t Ipad = round_up(std::max<int64_t>(I, 1), PAIRS_COL_ALIGN);

  // ---- the memory rule of run_pairs: Q and every block table resident, the query scratch bounded
  const double q_bytes = ((double)Ipad * S * KS + (double)Ipad * S) * sizeof(double);
  double t_bytes = 0.0;
  for (int side = 0; side < 2; side++)
    for (auto &b : p->blocks[side]) t_bytes += (double)b->M * (5 * KS + 3) * sizeof(double);
  {
    size_t free_b = 0, total_b = 0;
    const double frac = env_double("MFM_STORE_MAX_FRACTION", 0.5);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && q_bytes + t_bytes > frac * (double)free_b)
      throw Error(MFM_ERR_RUNTIME, "pair scoring: the candidate side's embedding (" + std::to_string((int64_t)(q_bytes / 1048576.0)) +
                                       " MB) and the block tables (" + std::to_string((int64_t)(t_bytes / 1048576.0)) +
                                       " MB) exceed MFM_STORE_MAX_FRACTION of the free device memory; score fewer candidates or smaller blocks per call");
  }
  const int64_t W = (I + 31) / 32;
  const int64_t steps_total = (std::max<int64_t>(I, 1) + form.step() - 1) / form.step();
  const double per_row = (double)S * KS * 8 + (double)(S + 1) * 8 + (p->has_exclude && !is_dense ? (double)W * 4 : 0.0) +
                         (is_dense ? (double)I * 16 : (double)(PAIRS_MAX_STRIPES + 1) * k * 12 + (double)k * 16);
  int64_t chunk = (int64_t)std::min<double>((double)p->scratch_bound / per_row, 1e12);
  chunk = std::max<int64_t>(chunk / PAIRS_ROW_ALIGN * PAIRS_ROW_ALIGN, PAIRS_ROW_ALIGN);
  chunk = std::min<int64_t>(chunk, round_up(U, PAIRS_ROW_ALIGN));

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
  const auto embed = [&](int side, const int64_t *ptr, const int32_t *ci, const double *val, int64_t r0, int64_t R, int64_t Rpad, double *Pf,
                         double *bias) {
    const dim3 grid((unsigned)((Rpad + PAIRS_WG - 1) / PAIRS_WG));
    const bool rel = !p->blocks[side].empty();
    const PairsVbBlockRef *blk = rel ? (const PairsVbBlockRef *)d_blk[side].p : nullptr;
    const int n_blk = (int)p->blocks[side].size();
    const auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(PAIRS_WG), 0, s, ptr, ci, val, r0, R, Rpad, pm, blk, n_blk, Pf, bias);
    };
    if (side == 1)
      rel ? launch(k_pairs_vb_embed<true, true>) : launch(k_pairs_vb_embed<false, true>);
    else
      rel ? launch(k_pairs_vb_embed<true, false>) : launch(k_pairs_vb_embed<false, false>);
  };

  // ---- candidate side, once
  DevBuf<double> Qf, Bb;
  Qf.alloc((size_t)std::max<int64_t>(Ipad * NK * 4, 1));
  Bb.alloc((size_t)Ipad * S);
  embed(1, p->c_ptr.p, p->c_idx.p, p->c_val.p, (int64_t)0, I, Ipad, Qf.p, Bb.p);
  MFM_HIP_CHECK(hipGetLastError());

  PairsArgs call;
  std::memset(&call, 0, sizeof(call));
  call.Qf = Qf.p;
  call.NK = NK;
  call.p_stride = NK;
  call.q_stride = NK;
  call.KS4 = KS4;
  call.S = S;
  call.Bb = Bb.p;
  call.w0s = d_w0.p;
  call.beta = mo.beta;
  call.Ipad = Ipad;
  call.I = I;
  call.W = W;
  call.k = k;

  // ---- queries, chunk by chunk
  DevBuf<double> Pf, Ab, list_v, out_v, d_dense, d_dense_std, out_m, out_s;
  DevBuf<int32_t> list_i, out_i;
  DevBuf<uint32_t> mask;
  std::vector<int32_t> h_idx;
  for (int64_t u0 = 0; u0 < U; u0 += chunk) {
    const int64_t Uc = std::min(chunk, U - u0), Upad = round_up(Uc, PAIRS_ROW_ALIGN);
    ensure(Pf, (size_t)(Upad * NK * 4));
    ensure(Ab, (size_t)(Upad * S));
    embed(0, p->q_ptr.p, p->q_idx.p, p->q_val.p, u0, Uc, Upad, Pf.p, Ab.p);
    MFM_HIP_CHECK(hipGetLastError());
    const bool use_mask = !is_dense && p->has_exclude && p->e_ptr_host[u0 + Uc] > p->e_ptr_host[u0];
    if (use_mask) {
      ensure(mask, (size_t)(Uc * W));
      MFM_HIP_CHECK(hipMemsetAsync(mask.p, 0, (size_t)(Uc * W) * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_pairs_mask, dim3((unsigned)((Uc + 3) / 4)), dim3(PAIRS_WG), 0, s, p->e_ptr.p, p->e_idx.p, u0, Uc, W, mask.p);
    }
    const int64_t n_qt = Upad / form.rows();
    int64_t n_stripes = std::max<int64_t>(1, std::min<int64_t>({(512 + n_qt - 1) / n_qt, steps_total, (int64_t)PAIRS_MAX_STRIPES}));
    const int64_t stripe_steps = (steps_total + n_stripes - 1) / n_stripes;
    n_stripes = (steps_total + stripe_steps - 1) / stripe_steps;
    const dim3 grid((unsigned)n_qt, (unsigned)n_stripes);
    PairsArgs a = call;
    a.Pf = Pf.p;
    a.Ab = Ab.p;
    a.Upad = Upad;
    a.Uc = Uc;
    a.stripe_len = stripe_steps * form.step();
    a.mask = use_mask ? mask.p : nullptr;
    a.list_rows = Upad;
    a.u0 = u0;
    if (is_dense) {
      ensure(d_dense, (size_t)(Uc * I));
      ensure(d_dense_std, (size_t)(Uc * I));
      a.dense = d_dense.p;
      a.dense_std = d_dense_std.p;
      form.launch(s, grid, a);
      MFM_HIP_CHECK(hipGetLastError());
      MFM_HIP_CHECK(hipMemcpyAsync(mo.sd + (size_t)u0 * I, d_dense_std.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipMemcpyAsync(dense + (size_t)u0 * I, d_dense.p, (size_t)(Uc * I) * sizeof(double), hipMemcpyDeviceToHost, s));
      MFM_HIP_CHECK(hipStreamSynchronize(s));
      continue;
    }
    ensure(list_v, (size_t)(n_stripes * Upad * k));
    ensure(list_i, (size_t)(n_stripes * Upad * k));
    ensure(out_v, (size_t)(Uc * k));
    ensure(out_i, (size_t)(Uc * k));
    ensure(out_m, (size_t)(Uc * k));
    ensure(out_s, (size_t)(Uc * k));
    a.list_v = list_v.p;
    a.list_i = list_i.p;
    if (I > 0) {
      form.launch(s, grid, a);
      MFM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_pairs_merge, dim3((unsigned)Uc), dim3(PAIRS_WG), 0, s, list_v.p, list_i.p, I > 0 ? (int)n_stripes : 0, Upad, k,
                       out_v.p, out_i.p);
    MFM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_pairs_vb_at, dim3((unsigned)((Uc * k + PAIRS_WG - 1) / PAIRS_WG)), dim3(PAIRS_WG), 0, s, a, out_i.p, Uc * k, out_m.p,
                       out_s.p);
    MFM_HIP_CHECK(hipGetLastError());
    h_idx.resize((size_t)(Uc * k));
    MFM_HIP_CHECK(hipMemcpyAsync(mo.mean + (size_t)u0 * k, out_m.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipMemcpyAsync(mo.sd + (size_t)u0 * k, out_s.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipMemcpyAsync(score + (size_t)u0 * k, out_v.p, (size_t)(Uc * k) * sizeof(double), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipMemcpyAsync(h_idx.data(), out_i.p, (size_t)(Uc * k) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    MFM_HIP_CHECK(hipStreamSynchronize(s));
    for (int64_t e = 0; e < Uc * k; e++) idx[u0 * k + e] = h_idx[(size_t)e];
  }
  MFM_HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace

extern "C" {

int mfm_pairs_moments_vb(mfm_pairs *p, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                         const double *V_var, double extra_var, double *mean, double *sd) {
  if (!p) {
    g_pairs_error = "mfm_pairs_moments_vb: no pair design";
    return MFM_ERR_INVALID;
  }
  PAIRS_TRY(p)
  if (!mean || !sd) throw Error(MFM_ERR_INVALID, "no output array");
  PairsMoments mo;
  mo.sd = sd;
  run_pairs_vb(p, PairsVbHost{rank, w0, w0_var, extra_var, w, w_var, V, V_var}, 0, nullptr, nullptr, mean, mo);
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
  const PairsMoments mo = checked_ucb(k, beta, idx, value, mean, sd);
  run_pairs_vb(p, PairsVbHost{rank, w0, w0_var, extra_var, w, w_var, V, V_var}, k, idx, value, nullptr, mo);
  PAIRS_CATCH(p)
}

}  // extern "C"
