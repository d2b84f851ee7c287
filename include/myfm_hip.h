/* myfm_hip.h -- C ABI of libmyfm_hip.so: the MI355X (gfx950) Gibbs-sampler hot path of
 * Bayesian Factorization Machines, as the host layer behind myFM's pybind11 boundary binds it.
 *
 * What this replaces in the reference (paths relative to /root/reference):
 *   the arithmetic of GibbsFMTrainer::update_all (include/myfm/BaseFMTrainer.hpp:135-152),
 *   i.e. include/myfm/FMTrainer.hpp:127-522, the scorer FM::predict_score_write_target
 *   (include/myfm/FM.hpp:54-136) and Predictor::predict* (include/myfm/predictor.hpp:35-147).
 * Who calls it: myfm_amd/csrc/_myfm.cpp -- a pybind11 module with the reference's names
 *   (cpp_source/declare_module.hpp:67-404) whose create_train_fm drives these entry points
 *   exactly where the reference's create_train_fm (declare_module.hpp:30-45) drives Eigen.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer argument is HOST memory owned by the
 *     caller and may be freed as soon as the call returns (the library copies / uploads);
 *   - the ctx owns all device memory and one HIP stream; one host thread per ctx;
 *   - matrices: CSR with int64 indptr, int32 indices, f64 data (scipy layout after
 *     base.py:285-286); dense V is column-major (D, K) like the reference
 *     (definitions.hpp:17), hyper matrices mu_V / lambda_V are column-major (G, K), i.e.
 *     element (g, f) at [f * G + g] (HyperParams.hpp:18-19);
 *   - every call returns MFM_OK or an error code; mfm_last_error() gives the message. The
 *     host layer maps MFM_ERR_INVALID -> ValueError (std::invalid_argument in the
 *     reference) and MFM_ERR_RUNTIME / MFM_ERR_DEVICE -> RuntimeError;
 *   - there is NO CPU fallback: without a usable HIP device mfm_create fails with
 *     MFM_ERR_DEVICE.
 */
#ifndef MYFM_HIP_H_
#define MYFM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFM_OK 0
#define MFM_ERR_INVALID 1 /* std::invalid_argument in the reference -> ValueError   */
#define MFM_ERR_RUNTIME 2 /* std::runtime_error in the reference    -> RuntimeError */
#define MFM_ERR_DEVICE 3  /* HIP failure / no device                -> RuntimeError */

/* task types: FMLearningConfig.hpp:14 (TASKTYPE) */
#define MFM_TASK_REGRESSION 0
#define MFM_TASK_CLASSIFICATION 1
#define MFM_TASK_ORDERED 2

typedef struct mfm_ctx mfm_ctx;       /* one training problem resident on one GPU            */
typedef struct mfm_design mfm_design; /* a (main CSR, relation blocks) design for prediction */
typedef struct mfm_store mfm_store;   /* posterior samples kept resident in HBM                */

/* ---- library / device ---------------------------------------------------------------- */
const char *mfm_version(void);
/* number of visible HIP devices; 0 when there is none (never fails). */
int mfm_device_count(void);
/* last error of a call that had no ctx (mfm_create, mfm_design_create) on this thread. */
const char *mfm_global_error(void);

/* ---- training context: replaces the BaseFMTrainer ctor, BaseFMTrainer.hpp:58-105 ------ */
int mfm_create(int device, mfm_ctx **out);
void mfm_destroy(mfm_ctx *ctx);
const char *mfm_last_error(const mfm_ctx *ctx);
int mfm_get_device(const mfm_ctx *ctx); /* the HIP device index the context lives on */
/* use an existing hipStream_t (e.g. torch's current stream) instead of the ctx's own. */
int mfm_set_stream(mfm_ctx *ctx, void *hip_stream);
int mfm_synchronize(mfm_ctx *ctx);

/* ---- row-sharded multi-GPU mode (one process per GPU) ---------------------------------
 * Every rank holds a contiguous slice of the training rows (its slice of X, y and of every
 * original_to_block) and a full replica of the model state, hyper-parameters and random variates.
 * `fn(user, dev_buf, count)` must sum `count` doubles at device address `dev_buf` IN PLACE over all
 * ranks, enqueued in order on the ctx stream (e.g. torch.distributed.all_reduce on the RCCL backend with
 * the ctx stream made current, see mfm_set_stream), and return 0. The library calls it once per level
 * of every sweep (2 |level| doubles), once per (block, factor) for the block statistics, and for
 * sum e / sum e^2 and the ordered-probit likelihood terms. Must be called before mfm_finalize.        */
int mfm_set_allreduce(mfm_ctx *ctx, int (*fn)(void *user, void *dev_buf, int64_t count), void *user);
/* ... with the callback provider: this rank's index and the number of ranks. REQUIRED together with mfm_set_allreduce
 * (mfm_comm_init implies it): rank 0 alone contributes the replicated columns to the model synchronisation after a
 * sharded latent sweep. A caller that never says (the older sequence mfm_set_allreduce + mfm_set_row_offset) is taken
 * to be the root exactly when its shard starts at global row 0.                                                       */
int mfm_set_shard(mfm_ctx *ctx, int32_t rank, int32_t world);
/* Native provider: RCCL called from this library on the ctx stream (ncclAllReduce, fp64 sum, in place) -- no callback,
 * no interpreter in the loop. One rank obtains the 128-byte id (ncclGetUniqueId) and hands it to the others by any
 * out-of-band means (e.g. a torch.distributed / MPI broadcast); every rank then calls mfm_comm_init (collective:
 * ncclCommInitRank on the ctx's device) before mfm_finalize. librccl.so is bound at run time.                          */
int mfm_comm_unique_id(void *out128);
int mfm_comm_init(mfm_ctx *ctx, const void *id128, int32_t rank, int32_t world);
/* collectives issued so far and doubles they carried (either provider) */
int mfm_comm_stats(const mfm_ctx *ctx, int64_t *calls, int64_t *doubles);
/* native provider: the communicator's own rank count (ncclCommCount) and the path of the librccl.so that was bound
 * (resolution order: one already mapped into the process, the directory of the HIP runtime in use, the loader's search
 * path, /opt/rocm/lib). n_ranks = 0 and an empty path when the ctx has no native communicator.                         */
int mfm_comm_info(const mfm_ctx *ctx, int32_t *n_ranks, char *path, int64_t path_cap);
/* Row-sharded persistent sweep (two-field one-hot table, shards cut between users): mfm_finalize builds the sweep's layout on every
 * rank and allocates the rank's exchange buffers; the sweep goes live once every rank knows every rank's buffers -- until then the
 * per-factor passes run. Inside the launch a rank writes its item sums into every peer's buffer and raises a flag there (no
 * collective between the launches; SURVEY 8e "one-shot all-reduce"). mfm_peer_info: is a layout waiting (pending), this rank's
 * buffers. mfm_peer_set: all ranks' device pointers, valid on THIS device (ranks in one process, or mapped by the caller).
 * mfm_peer_export / mfm_peer_import: the same through IPC handles for one process per GPU (256 bytes per rank: sums, flags, w, V; exchanged by the
 * caller over any channel). Every rank must make the same calls between the same two sweeps.                                  */
int mfm_peer_info(mfm_ctx *ctx, int32_t *pending, void **sum_buf, void **flag_buf, int64_t *sum_bytes, int64_t *flag_bytes);
int mfm_peer_set(mfm_ctx *ctx, int32_t world, int32_t rank, void *const *sum_bufs, void *const *flag_bufs);
/* optional, after mfm_peer_set: every rank's w / V (mfm_peer_model_info gives this rank's). A first-level coefficient is then written
 * to every replica where and when it is drawn, and the model synchronisation after the launch (an all-reduce of w and V) is dropped. */
int mfm_peer_model_info(mfm_ctx *ctx, void **w_buf, void **V_buf);
int mfm_peer_set_model(mfm_ctx *ctx, int32_t world, int32_t rank, void *const *w_bufs, void *const *V_bufs);
int mfm_peer_export(mfm_ctx *ctx, void *handles256);
int mfm_peer_import(mfm_ctx *ctx, int32_t world, int32_t rank, const void *all_handles);
/* give it up (waiting or live): the per-factor passes from the next sweep on; every rank alike */
int mfm_peer_drop(mfm_ctx *ctx);
/* The level schedule of the main table's columns (mfm_host_column_levels of the GLOBAL design): in the
 * row-sharded mode it must be identical on every rank (a conflict may exist only in another rank's
 * rows), so the caller computes it before sharding. Checked against the local rows at mfm_finalize.
 * Relation-block matrices are replicated, their schedules need no hand-over.                          */
int mfm_set_main_levels(mfm_ctx *ctx, const int32_t *level, int64_t D0);
/* global index of this rank's first row: keys the per-row Philox streams so that the latent draws of
 * classification / ordered probit do not depend on how the rows are sharded.                         */
int mfm_set_row_offset(mfm_ctx *ctx, int64_t first_global_row);

/* main table X (N x D0) and targets y[N]; D0 may be 0 (base.py:230-233). The arrays are validated and copied to the device
 * before the call returns (no host copy is kept); the caller may free them afterwards.                                      */
int mfm_set_main(mfm_ctx *ctx, int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices,
                 const double *data, const double *y);
/* RelationBlock (definitions.hpp:30-52): block CSR (B x Db) + original_to_block[N].
 * MFM_ERR_RUNTIME "index mapping points to non-existing row." on a bad index (:38-41).    */
int mfm_add_block(mfm_ctx *ctx, int64_t B, int64_t Db, const int64_t *indptr, const int32_t *indices,
                  const double *data, const int64_t *original_to_block);
/* group_index over ALL D = D0 + sum Db features (FMLearningConfig.hpp:83), G groups.      */
int mfm_set_groups(mfm_ctx *ctx, const int32_t *group_index, int64_t D, int32_t G);
/* recomputable = 1 (regression): outside the sweeps the residual is always e = score - y -- mfm_update_e_regression follows every
 * update_V (FMTrainer.hpp:494) -- so a sweep that keeps the residual on chip need not write its copy back; whoever reads the
 * residual between the sweep and the update gets it recomputed (equal up to rounding). Default 0: every sweep leaves its residual. */
int mfm_set_residual_policy(mfm_ctx *ctx, int32_t recomputable);
/* Builds the device-side design: CSC (= X_t, BaseFMTrainer.hpp:61), the conflict-free level
 * schedule of the columns, the residual/q-cache vectors. rank = n_factors (may be 0).      */
int mfm_finalize(mfm_ctx *ctx, int32_t rank);

int64_t mfm_dim_all(const mfm_ctx *ctx);
/* schedule statistics: number of main-table levels, of main-table kernel launches per sweep */
int mfm_plan_info(const mfm_ctx *ctx, int64_t *n_levels_main, int64_t *n_launches_per_sweep);
/* Which fast paths mfm_finalize selected for the main table (diagnostics / tests):
 * bit 0 = q-free latent sweep (short rows: q_train is recomputed, not stored, during update_V),
 * bit 1 = all stored values are 1.0 (values never read), bit 2 = uniform row length (rowptr never read),
 * bit 3 = row-sharded (mfm_set_allreduce), bit 4 = split e / q arrays during update_V,
 * bit 5 = the last level's apply pass also runs the next factor's first level (k_tile_apply_next),
 * bit 6 = row-sharded with the fused tile path (first-level columns swept where their rows live),
 * bit 7 = two-field pass (two one-hot-like levels: one pass over the residual per factor, no q-cache in HBM),
 * bit 8 = persistent latent sweep (residual on chip for update_w + update_V), bit 9 = index-tuple designs (cell passes),
 * bit 10 = a relation block's feature chain (FMTrainer.hpp:276-302, :419-470) runs as the streamed one-launch form,
 * bit 11 = the persistent sweep holds more rows per CU than fit on chip (the rest of the residual is streamed every sweep). */
int mfm_plan_flags(const mfm_ctx *ctx);
/* The persistent sweep's slot layout (csrc/mfm_res.hpp, ResPlan) as mfm_finalize left it, for diagnostics and for tests that must
 * prove which layout edge they reached. Reads host-side fields only: no launch, no synchronisation. out[i], i < n_out:
 *   0 ready (the layout was taken), 1 G (workgroups), 2 RV / 3 RL / 4 RX (slots per thread in registers / in LDS / streamed from
 *   global memory), 5 umax (stride of the per-wave accumulator arrays), 6 n_items, 7 item_bits, 8 n_runs ((workgroup, item) pairs),
 *   9 the most first-level columns any workgroup draws, 10 the most items any slice draws, 11 where the residual is now
 *   (0 row order, 1 slot order, 2 slot order with its sums from mfm_update_e_regression, 3 cell order, 4 not stored: recomputed on
 *   demand), 12 the rows the layout was planned for, 13 the kernel form (0: the user level's sum of h^2 is taken in sweep A, 1: in
 *   sweep B of the sweep before, with a third accumulator array in LDS), 14 the kernel's dynamic LDS in bytes, 15 the bytes of an entry of the item draw's
 *   lists (4: run and item packed into one word, 8: two words; csrc/mfm_res_entry.hpp); entries beyond
 *   MFM_RES_INFO_FIELDS are 0. Fields 1-10 and 13-15 are those of the last
 *   layout the planner tried: after a refusal the ones it had not reached keep their earlier values (0 in a fresh context).
 * why (why_len bytes, NUL-terminated, may be NULL with why_len 0): the planner's refusal text when not ready, else empty. */
#define MFM_RES_INFO_FIELDS 16
int mfm_res_info(const mfm_ctx *ctx, int64_t *out, int n_out, char *why, int why_len);
/* The cell path's plan (csrc/mfm_cell.hpp, CellPlan: index-tuple designs) as mfm_finalize left it, for diagnostics and for tests
 * that must prove which layout edge they reached. Reads host-side fields only: no launch, no synchronisation. out[i], i < n_out:
 *   0 ready (the plan was taken), 1 G (groups = workgroups of a pass), 2 umax (most first-field values of one group), 3 item32 (the
 *   scattered index is a separate int32 array), 4 n_streams, 5 n_fields, 6 N, 7 Npad (positions of the padded step layout),
 *   8 the most steps any group takes, 9 / 10 rows of the longest / the shortest wave chunk (an empty chunk counts as 0), 11 wave
 *   chunks without a row, 12 bit k set: update_V's pass into field k (apply the field before it, statistics of k) runs as an
 *   apply-only launch plus a statistics-only launch because both roles do not fit the LDS together, 13 factors per pass of the
 *   scorer (4, 2 or 1; 0 when not ready);
 *   14 + 3 s ..: stream s < 4: type (0 U: sorted first field, 1 I: the scattered stream, 2 C: whole table in LDS), its 16-bit slot of
 *   the row record (-1: the int32 array), its cardinality;   26 + 3 k ..: field k < 16 in Gibbs order: its stream, its kind (0 one-hot
 *   main field, 1 relation block), its columns / block rows. Entries of streams and fields that do not exist, and entries beyond
 *   MFM_CELL_INFO_FIELDS, are 0. The fields are those of the last plan the planner tried: after a refusal the ones it had not
 *   reached keep their earlier values (0 in a fresh context, and in one whose design the cell path was never tried on).
 * why (why_len bytes, NUL-terminated, may be NULL with why_len 0): the planner's refusal text when not ready (empty when the cell
 * path was not tried), else empty. */
#define MFM_CELL_INFO_FIELDS 74
int mfm_cell_info(const mfm_ctx *ctx, int64_t *out, int n_out, char *why, int why_len);
/* The streamed chain runs (csrc/mfm_chain_stream.hpp, k_cs_stream) of the relation blocks' plans as mfm_finalize left them, and how
 * often each has been launched, for diagnostics and for tests that must prove which plan ran and which of the kernel's paths it
 * reached. Reads host-side fields only: no launch, no synchronisation. One record of MFM_CHAIN_STREAM_INFO_FIELDS entries per
 * streamed run, blocks in the order they were added, runs in sweep order; at most max_records are written to out, *n_records (may be
 * NULL) is the number there are. A record:
 *   0 block, 1 columns of the run, 2 steps, 3 Cg (columns per step), 4 Lw (window in steps), 5 NB (row ranges), 6 RD (slot reuse
 *   delay), 7 LDS slots, 8 most hot entries of a column, 9 / 10 most rows entering / leaving the LDS in a step, 11 / 12 / 13 most
 *   cold entries / entering rows / leaving rows of one (step, range), 14 columns without a hot entry, 15 + i, i < 10: columns whose
 *   hot entries fill min(ceil(hot / 64), 9) = i wavefront rounds, 25 the walker workgroup's dynamic LDS in bytes, 26 cold entries,
 *   27 hot entries, 28 / 29 launches enqueued so far by update_w / by update_V (one per factor), counted on the host.           */
#define MFM_CHAIN_STREAM_INFO_FIELDS 30
int mfm_chain_stream_info(const mfm_ctx *ctx, int64_t *out, int max_records, int *n_records);

/* ---- model state (FM.hpp:164-168) ------------------------------------------------------ */
int mfm_set_state(mfm_ctx *ctx, double w0, const double *w, const double *V);
int mfm_get_state(mfm_ctx *ctx, double *w0, double *w, double *V);
int mfm_set_w0(mfm_ctx *ctx, double w0); /* scalar only; does not touch e (FMTrainer.hpp:219-222) */
int mfm_zero_w(mfm_ctx *ctx);            /* fit_linear == false, FMTrainer.hpp:232-235            */
/* residual e_train and per-factor cache q_train (BaseFMTrainer.hpp:46-47), for tests.      */
int mfm_get_e(mfm_ctx *ctx, double *e);
int mfm_get_q(mfm_ctx *ctx, double *q);
int mfm_set_e(mfm_ctx *ctx, const double *e);

/* ---- the Gibbs iteration, in update_all order (BaseFMTrainer.hpp:135-152) --------------- */
/* sum_t e_t and sum_t e_t^2 : inputs of update_alpha (FMTrainer.hpp:138) and update_w0
 * (:223, sum(w0 - e) = N w0 - sum e).                                                       */
int mfm_reduce_e(mfm_ctx *ctx, double *sum_e, double *sum_e2);
/* e += delta (FMTrainer.hpp:227).                                                           */
int mfm_shift_e(mfm_ctx *ctx, double delta);
/* per-group sufficient statistics of w for update_lambda_w / update_mu_w
 * (FMTrainer.hpp:150-200): sum[g] = sum_{j in g} w_j, ssd[g] = sum_{j in g} (w_j - mu[g])^2 */
int mfm_group_stats_w(mfm_ctx *ctx, const double *mu_w, double *sum, double *ssd);
/* same for every factor of V (FMTrainer.hpp:202-216); all arrays (G, K) column-major.       */
int mfm_group_stats_V(mfm_ctx *ctx, const double *mu_V, double *sum, double *ssd);
/* reduce_e + group_stats_w + group_stats_V with one host synchronisation (same outputs; need_e = 0 skips the
 * residual sums). All three only read state the iteration has not touched yet when it needs them
 * (FMTrainer.hpp:138, :150-216, :223). (G) and (G, K) arrays are column-major like the reference's. */
int mfm_hyper_stats(mfm_ctx *ctx, int32_t need_e, const double *mu_w, const double *mu_V, double *sum_e, double *sum_e2,
                    double *sum_w, double *ssd_w, double *sum_V, double *ssd_V);
/* update_w (FMTrainer.hpp:231-314): main table then relation blocks, feature order preserved
 * for every pair of features that share a row. z[D] = the N(0,1) variates of the D
 * sample_normal calls in reference order (main columns, then each block's columns); z == NULL uses the
 * device-generated variates of the set acquired by mfm_rng_acquire.                          */
int mfm_sweep_w(mfm_ctx *ctx, double alpha, const double *lambda_w, const double *mu_w, const double *z);
/* update_V (FMTrainer.hpp:316-486) for factors [f_begin, f_end): per factor the q-cache build
 * (:320-340), the main-table sweep (:343-376) and the per-block sweeps (:378-482).
 * lambda_V / mu_V: full (G, K) column-major; z: (f_end - f_begin) * D variates, factor-major. */
int mfm_sweep_V(mfm_ctx *ctx, int32_t f_begin, int32_t f_end, double alpha, const double *lambda_V,
                const double *mu_V, const double *z);
/* update_w0's residual shift (FMTrainer.hpp:226: e += e_shift), update_w (:231-314) and update_V (:316-486) of factors
 * [f_begin, f_end) as ONE call: BaseFMTrainer.hpp:143-148 draws lambda_V / mu_V between the two sweeps, but those draws read
 * neither w nor e, so the caller can make them first. Same results as mfm_shift_e + mfm_sweep_w + mfm_sweep_V; on a
 * two-field one-hot table it is one persistent launch. zw / zv: both NULL (the acquired device random set) or both given. */
int mfm_sweep_wV(mfm_ctx *ctx, double alpha, double e_shift, const double *lambda_w, const double *mu_w, const double *zw,
                 int32_t f_begin, int32_t f_end, const double *lambda_V, const double *mu_V, const double *zv);

/* One WHOLE regression iteration (GibbsFMTrainer::update_all, BaseFMTrainer.hpp:135-152) enqueued without a host round trip inside
 * it: the reductions update_alpha / update_w0 / update_lambda_* / update_mu_* need (FMTrainer.hpp:127-229), those conditionals
 * themselves on the device (k_hyper_regression: the trainer's arithmetic, operation for operation, on the unit variates of the
 * acquired random set -- draw program [gamma: alpha][normal: w0 if fit_w0][G gammas: lambda_w][G normals: mu_w][K G gammas:
 * lambda_V][K G normals: mu_V] + the w and V sweep normals), update_w0's shift + update_w + update_V as the persistent launch
 * (:231-486), the request for the set after the next, update_e (:493-497). With the host in the loop (mfm_hyper_stats -> host
 * draws -> mfm_sweep_wV) every iteration paid ~0.1 ms of read-back / upload / dispatch latency between two launches.
 *   prior: alpha_0, beta_0, gamma_0, mu_0, reg_0 of FMLearningConfig, n_total = training rows, fit_w0; n_in_group: [G] features
 *   per group. In: *w0, mu_w, mu_V = the current values. Out: this iteration's draws (the call returns when they have arrived,
 *   i.e. early in the iteration's device work: w / V / e are still being swept, like after mfm_sweep_wV).
 *   Errors raised ON the device by this iteration's own launches (a co-residency time-out of the persistent sweep, an exhausted
 *   random stream) cannot be known when the call returns: they are returned by the NEXT call that waits for the stream -- the next
 *   mfm_regression_iteration, mfm_get_state, mfm_synchronize -- and always before a model leaves the device.
 * mfm_regression_iteration_ready: 1 when the context can do this now (finalized two-field table on the persistent sweep, one GPU,
 * the residual in the sweep's slot order with its sums from the last mfm_update_e_regression, a device random stream programmed
 * as above); else 0 and the caller runs the iteration step by step. */
typedef struct mfm_hyper_prior {
  double alpha_0, beta_0, gamma_0, mu_0, reg_0, n_total;
  int32_t fit_w0, reserved;
} mfm_hyper_prior;
int mfm_regression_iteration_ready(mfm_ctx *ctx);
int mfm_regression_iteration(mfm_ctx *ctx, const mfm_hyper_prior *prior, const double *n_in_group, double *alpha, double *w0,
                             double *lambda_w, double *mu_w, double *lambda_V, double *mu_V);
/* update_e (FMTrainer.hpp:493-522), regression: e = predict_score(X_train) - y.             */
int mfm_update_e_regression(mfm_ctx *ctx);
/* update_e, probit classification (:498-512): e_t = score_t - z_t, z_t ~ TN(score_t, 1) on
 * (0, inf) if y_t > 0 else (-inf, 0) (util.hpp:15-78). The reference consumes its mt19937 in
 * data-dependent rejection loops; here each row draws from a Philox4x32-10 stream keyed by
 * (seed, draw_index, row): parity is distributional.                            */
int mfm_update_e_classification(mfm_ctx *ctx, uint64_t seed, uint64_t draw_index);
/* e = predict_score(X_train) only (initialize_e for the ordered task, FMTrainer.hpp:100).   */
int mfm_score_train(mfm_ctx *ctx);

/* ordered probit (OProbitSampler.hpp): one cutpoint group = a row subset with n_class labels.
 * rows == NULL means all N rows. Returns the group id in *group.                            */
int mfm_oprobit_add_group(mfm_ctx *ctx, int32_t n_class, const int64_t *rows, int64_t n_rows, int32_t *group);
/* log-likelihood, d/dgamma and the gamma-space Hessian accumulators of
 * OprobitSampler::operator() (OProbitSampler.hpp:402-413, 111-236) over the group's rows at
 * cutpoints gamma[n_class-1], on the current e (= score). H is (n_class-1)^2 row-major; pass
 * NULL to skip it.                                                                          */
int mfm_oprobit_eval(mfm_ctx *ctx, int32_t group, const double *gamma, double *ll, double *dgamma, double *H);
/* sample_z_given_cutpoint (OProbitSampler.hpp:238-272): e_t -= z_t, Philox-keyed as above.  */
int mfm_oprobit_sample_z(mfm_ctx *ctx, int32_t group, const double *gamma, uint64_t seed, uint64_t draw_index);

/* ---- device-side random stream (bit-compatible with the reference's std::mt19937 + libstdc++
 * distributions, see csrc/mfm_rng.hpp) ----------------------------------------------------------
 * For regression / classification the engine outputs consumed per Gibbs iteration do not depend on
 * the model state, so the iteration's variates are produced on the GPU ahead of the sweeps:
 *   - mfm_rng_seed_mt19937: hand over the generator (the 624 state words and the position index of
 *     a std::mt19937, e.g. after FM::initialize_weight consumed its share, FM.hpp:34-45);
 *   - mfm_rng_set_program: the draw order of one iteration as a list of ops (SURVEY 8a "RNG draw
 *     order"): NORMALS(count) = that many `sample_normal` variates (FMTrainer.hpp:122-125: a fresh
 *     normal_distribution per draw), GAMMA(shape) = the unit-scale variate of
 *     gamma_distribution(shape, scale) (FMTrainer.hpp:142-143, :164-165; multiply by scale);
 *     dest 0 = "hyper" variates returned to the host in program order, 1 = z of mfm_sweep_w (D),
 *     2 = z of mfm_sweep_V (K * D, factor-major);
 *   - mfm_rng_prefetch: start producing a further iteration's variates on a side stream. Sets are produced in
 *     iteration order; up to two may be in flight besides the acquired one (the trainer requests the set of
 *     iteration t + 2 right after the latent sweep of iteration t is enqueued). Where the persistent sweep fills the
 *     device, a set with another one ahead of it is produced in two parts: its single-workgroup kernels (generator,
 *     hyper draws, the linear term's normals) right away, beside the sweep; its whole-GPU evaluation of the K D
 *     sweep normals with the NEXT mfm_rng_prefetch (or the mfm_rng_acquire that needs it), behind everything
 *     enqueued on the ctx stream by then -- between two sweeps, not starved beside one;
 *   - mfm_rng_acquire: wait for the oldest prefetched set, copy its hyper variates to the host and
 *     make its z buffers the ones mfm_sweep_w / mfm_sweep_V use when called with z == NULL.      */
#define MFM_RNG_NORMALS 0
#define MFM_RNG_GAMMA 1
/* MFM_RNG_LATENT(count = rows): not a draw of the set -- tells the generator that every iteration also consumes about 6 outputs per
 * row through mfm_update_e_classification_exact / mfm_oprobit_sample_z_exact (sizes the ring and the parallel generator).        */
#define MFM_RNG_LATENT 2
typedef struct mfm_rng_op {
  int32_t kind;   /* MFM_RNG_NORMALS | MFM_RNG_GAMMA | MFM_RNG_LATENT      */
  int32_t dest;   /* 0 hyper variates, 1 z_w, 2 z_V                        */
  int64_t count;  /* NORMALS: number of draws; GAMMA: 1                    */
  int64_t offset; /* first index in the destination                        */
  double shape;   /* GAMMA: alpha                                          */
} mfm_rng_op;
/* Optional, no context needed: start computing the parallel generator's jump-ahead polynomials for a problem of this size on a
 * helper thread (cached per process; mfm_finalize asks for the same ones, so a caller that knows (D, rank, groups) before the
 * design is handed over hides the ~0.1-0.3 s they take behind its own setup).                                                */
int mfm_rng_prepare(int64_t n_features, int32_t rank, int32_t n_groups);
int mfm_rng_seed_mt19937(mfm_ctx *ctx, const uint32_t *state624, int32_t position);
int mfm_rng_set_program(mfm_ctx *ctx, const mfm_rng_op *ops, int32_t n_ops);
int mfm_rng_prefetch(mfm_ctx *ctx);
int mfm_rng_acquire(mfm_ctx *ctx, double *hyper_variates, int64_t n_hyper_variates);
/* test hook: the z buffers of the acquired set (zw[D], zv[K*D]); either pointer may be NULL. */
int mfm_rng_get_z(mfm_ctx *ctx, double *zw, double *zv);

/* ---- the draws the reference makes in a state-dependent order, on the SAME device stream ("exact" latent mode) ----
 * The latent z of probit classification (FMTrainer.hpp:498-512) and ordered probit (OProbitSampler.hpp:238-272) consume the
 * generator row after row inside rejection loops (util.hpp:15-60). These two entry points make exactly those draws from the
 * stream's current position -- same variates for the same rows, same number of engine outputs consumed -- evaluated in parallel
 * (csrc/mfm_latent.hip). No set may be in flight (acquire what was prefetched first); the next mfm_rng_prefetch starts where
 * the draw ended. *status: 0 = done. Otherwise NOTHING was drawn or consumed (e still holds the scores) and the caller makes
 * the draws sequentially through mfm_rng_host_read / mfm_rng_host_advance: 1 = the true path left a chunk's window of
 * candidate rows even at +-6.5 sigma (probability ~1e-8 per call), 2 / 3 = scratch space, 4 = more engine outputs needed than
 * prepared, 5 = a score more than 1000 standard deviations on the wrong side of its class.
 * mfm_update_e_classification_exact = FM::predict_score_write_target + the draws (the exact twin of
 * mfm_update_e_classification); mfm_oprobit_sample_z_exact = sample_z_given_cutpoint for one cutpoint group on the current e. */
int mfm_update_e_classification_exact(mfm_ctx *ctx, int32_t *status);
/* The order in which mfm_update_e_classification_exact serves the rows (FMTrainer.hpp:500 walks the caller's rows 0 .. N - 1): entry i =
 * the row of this table that is the caller's row i, for a caller that handed the rows over in another order (sorted for the device
 * paths). n = 0: the table's own order. (Ordered probit: the group's row list of mfm_oprobit_add_group is that order.)              */
int mfm_set_latent_order(mfm_ctx *ctx, const int64_t *rows, int64_t n);
int mfm_oprobit_sample_z_exact(mfm_ctx *ctx, int32_t group, const double *gamma, int32_t *status);
/* diagnostics of the last exact draw: {status, chunks, sub-chunks per chunk, quads per chunk, quads consumed, walkers started,
 * attempts (2: the first attempt's windows of +-3.5 sigma missed the path, the second's +-6.5 sigma held it), reserved} */
int mfm_latent_stats(mfm_ctx *ctx, int64_t *out8);
/* The host's window into the device stream: out[0..n) = the engine outputs (tempered, as std::mt19937::operator() returns them)
 * number offset .. offset + n - 1 counted from the stream's position; mfm_rng_host_advance moves the position by `words` outputs.
 * For the few draws the host makes itself between two sets (the cutpoint sampler's Metropolis step, OProbitSampler.hpp:55-72,
 * :378) and for the sequential fall-back of the two calls above. No set may be in flight.                                      */
int mfm_rng_host_read(mfm_ctx *ctx, uint64_t offset, int64_t n, uint32_t *out);
int mfm_rng_host_advance(mfm_ctx *ctx, uint64_t words);

/* ---- per-kernel timing (HIP events on the ctx stream) for bench.py's roofline block ---- */
int mfm_timing_enable(mfm_ctx *ctx, int on);
/* Restrict the event bracketing to one kernel class (index as in mfm_timing_class_name; < 0: all classes).
 * Bracketing every launch costs ~10 % at config 3; one class is cheap enough for a timed benchmark region. */
int mfm_timing_select(mfm_ctx *ctx, int32_t kernel_class);
int mfm_timing_reset(mfm_ctx *ctx);
int mfm_timing_n_classes(void);
const char *mfm_timing_class_name(int cls);
/* total milliseconds, launch count and algorithmic bytes (SURVEY 8d per-unit figures times
 * the units each launch processed) accumulated for one kernel class since the last reset.   */
int mfm_timing_get(mfm_ctx *ctx, int cls, double *ms_total, int64_t *launches, double *alg_bytes_total);

/* ---- prediction: FM::predict_score (FM.hpp:47-136), Predictor::predict* (predictor.hpp) -- */
int mfm_design_create(int device, int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices,
                      const double *data, mfm_design **out);
int mfm_design_add_block(mfm_design *d, int64_t B, int64_t Db, const int64_t *indptr, const int32_t *indices,
                         const double *data, const int64_t *original_to_block);
void mfm_design_destroy(mfm_design *d);
const char *mfm_design_last_error(const mfm_design *d);
int64_t mfm_design_dim_all(const mfm_design *d);
int64_t mfm_design_n_rows(const mfm_design *d);
/* mode 0: out[N]  = mean_s score_s                    (Predictor::predict, regression)
 * mode 1: out[N]  = mean_s Phi(score_s)               (classification, predictor.hpp:138-143)
 * mode 2: out[N * (n_cut + 1)] row-major = mean_s ordered-probit class probabilities with
 *         cutpoints[s * n_cut + c]                    (FM.hpp:137-162, predictor.hpp:78-124)
 * w0s[S], ws[S * D], Vs[S * D * K] (each sample's V column-major (D, K)).                   */
int mfm_design_predict(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws,
                       const double *Vs, int32_t mode, int32_t n_cut, const double *cutpoints, double *out);

/* ---- device-resident posterior samples: the Predictor's `samples` (FMTrainer.hpp:71-74, predictor.hpp:35-147) ------
 * mfm_store_push_ctx appends the live (w0, w, V) of a training context with a device-to-device copy on its stream (no
 * host transfer inside the Gibbs loop); mfm_store_get materialises one sample on the host (w[D], V column-major (D, K));
 * mfm_design_predict_store = mfm_design_predict over samples [first, first + count) read in place (cutpoints[count *
 * n_cut] for mode 2).                                                                                                */
int mfm_store_create(int device, int64_t D, int32_t rank, mfm_store **out);
void mfm_store_destroy(mfm_store *st);
const char *mfm_store_last_error(const mfm_store *st);
int32_t mfm_store_size(const mfm_store *st);
int mfm_store_reserve(mfm_store *st, int32_t n_samples); /* allocate room for n_samples ahead of the loop (optional) */
int mfm_store_push_ctx(mfm_store *st, mfm_ctx *ctx);
int mfm_store_push_host(mfm_store *st, double w0, const double *w, const double *V);
int mfm_store_get(mfm_store *st, int32_t idx, double *w0, double *w, double *V);
int mfm_design_predict_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t n_cut,
                             const double *cutpoints, double *out);

/* ---- posterior predictive summaries over the kept samples (csrc/mfm_dist.hpp) ------------------------------
 * Per design row, over samples [first, first + count) of a store (or n_samples host samples in the layout of
 * mfm_design_predict), with v_s = score_s (mode 0) or Phi(score_s) (mode 1):
 *   out_mean[N]       (v_0 + v_1 + ...) * (1 / S): bit for bit what mfm_design_predict* returns
 *   out_std[N]        population standard deviation of the v_s; with precisions sqrt(var_s + mean_s 1 / precisions[s])
 *   out_q[n_q * N]    row-major (n_q, N): the empirical quantile of the v_s at probs[q] under numpy's "linear" rule (exact
 *                     order statistics, sorted on the device); with precisions[S] (mode 0 only; z[q] = Phi^-1(probs[q]), probs
 *                     strictly inside (0, 1)) the quantile of the mixture mean_s N(score_s, 1 / precisions[s])
 * n_q <= 32; n_q > 0 needs count <= 4096 (MFM_ERR_INVALID otherwise); n_q = 0 computes the moments alone, for any count.
 * precisions / z may be NULL (no noise). tile_rows / chunk_samples force the row tile and the sample chunk of the device passes
 * (0: automatic); the results do not depend on them. mfm_design_summary uploads all its samples at once, S * D * (K + 1) * 8 bytes,
 * under the limit of mfm_store_reserve (MFM_ERR_RUNTIME beyond it).                                                         */
int mfm_design_summary_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t n_q,
                             const double *probs, const double *precisions, const double *z, int64_t tile_rows,
                             int32_t chunk_samples, double *out_mean, double *out_std, double *out_q);
int mfm_design_summary(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t mode, int32_t n_q, const double *probs, const double *precisions, const double *z,
                       int64_t tile_rows, int32_t chunk_samples, double *out_mean, double *out_std, double *out_q);
/* Ordered probit: the same summaries of a function of the score and of THAT sample's cutpoints, cutpoints[count * n_cut] row-major
 * (count, n_cut), with cdf_j = (1 + erf((cut_j - score) / sqrt 2)) / 2, cdf_-1 = 0, cdf_n_cut = 1 and C = n_cut + 1 classes:
 *   expected = 0: v_s[c] = p_c = cdf_c - cdf_c-1 per class; out_mean / out_std row-major (N, C), out_q row-major (n_q, N, C);
 *                 out_mean is bit for bit what mfm_design_predict* returns in mode 2
 *   expected = 1: v_s = sum_c c p_c, added in ascending class order; out_mean[N], out_std[N], out_q row-major (n_q, N)
 * There is no noise form (y is discrete: its predictive distribution is the out_mean of expected = 0) and no limit on C. n_cut < 1,
 * a cutpoint that is not finite and cutpoints that do not ascend within a sample are MFM_ERR_INVALID; n_q, count, tile_rows,
 * chunk_samples and the upload rule of the host flavour are those of mfm_design_summary*.                                   */
int mfm_design_summary_oprobit_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t expected, int32_t n_cut,
                                     const double *cutpoints, int32_t n_q, const double *probs, int64_t tile_rows,
                                     int32_t chunk_samples, double *out_mean, double *out_std, double *out_q);
int mfm_design_summary_oprobit(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                               int32_t expected, int32_t n_cut, const double *cutpoints, int32_t n_q, const double *probs,
                               int64_t tile_rows, int32_t chunk_samples, double *out_mean, double *out_std, double *out_q);

/* ---- pointwise log predictive density over the kept samples (csrc/mfm_logdens.hpp) --------------------------
 * Per design row t with observed target y[t], over the samples of mfm_design_summary*, l_s = log p(y[t] | sample s):
 *   task 0 (regression)      log N(y; score_s, 1 / precisions[s])
 *   task 1 (probit)          log Phi(score_s) for y = 1, log Phi(-score_s) for y = 0
 *   task 2 (ordered probit)  log(Phi(cut_s[y] - score_s) - Phi(cut_s[y - 1] - score_s)), cut_s[-1] = -inf, cut_s[n_cut] = +inf,
 *                            cutpoints[count * n_cut] row-major (count, n_cut)
 * evaluated without forming Phi (finite and relatively accurate to |score| ~ 38 and beyond).
 *   out_lpd[N]   logsumexp_s l_s - log S, the log pointwise predictive density
 *   out_mean[N]  mean_s l_s;   out_var[N]  the sample variance (ddof = 1) of the l_s, exactly 0 for S = 1 or equal values
 *   out_pit[N]   task 0 only, may be NULL: mean_s Phi((y - score_s) sqrt(precisions[s]))
 *   out_ll[S * N]  may be NULL: row-major (S, N), the l_s themselves
 * Everything is fp64 and summed in sample order: tile_rows / chunk_samples (0: automatic) do not change a bit of the results.
 * MFM_ERR_INVALID, before the device is used: a bad task; y not finite, not 0 / 1 (task 1), not an integer in [0, n_cut]
 * (task 2); precisions missing, non-positive or non-finite for task 0 or given otherwise; cutpoints missing (or n_cut < 1),
 * non-finite or not ascending for task 2 or given otherwise; out_pit for a task other than 0; negative tiling overrides. N = 0
 * returns at once. The upload rule of the host flavour is that of mfm_design_summary.                                        */
int mfm_design_logdens_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                             const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                             int32_t chunk_samples, double *out_lpd, double *out_mean, double *out_var, double *out_pit,
                             double *out_ll);
int mfm_design_logdens(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                       int64_t tile_rows, int32_t chunk_samples, double *out_lpd, double *out_mean, double *out_var,
                       double *out_pit, double *out_ll);
/* l of one (y, score) on the host, by the code the kernel runs (no device): log_norm = log(precision) / 2 - log(2 pi) / 2 and
 * sqrt_alpha for task 0, cutpoints_row[n_cut] for task 2, ignored otherwise                                                 */
int mfm_logdens_value(int32_t task, double y, double score, double log_norm, double sqrt_alpha, int32_t n_cut,
                      const double *cutpoints_row, double *out);

/* ---- Pareto-smoothed importance-sampling leave-one-out over the kept samples (csrc/mfm_psis.hpp) -------------
 * Per design row t, with l_s of mfm_design_logdens* and the importance ratios r_s = -l_s - max_s(-l_s): the largest tail_len
 * ratios (ordered by (r_s, s)) are replaced by the quantiles of a generalized Pareto distribution fitted to them (Zhang and
 * Stephens 2009 on a grid of 30 + floor(sqrt(tail_len)) points, the loo package's priors), lw_s = r_s - logsumexp_s r_s.
 *   out_elpd[N]  logsumexp_s(lw_s + l_s), the leave-one-out log predictive density when y[t] is a row the model was fitted on
 *   out_k[N]     the fit's shape k^; +inf where no fit was made: tail_len < 5, a tail whose lower quarter equals the cutoff,
 *                or an l_s of -inf (then out_elpd = -inf and the row's log weights are NaN)
 *   out_lpd[N]   as mfm_design_logdens* writes it, bit for bit
 *   out_pit[N]   task 0 only, may be NULL: sum_s exp(lw_s) Phi((y - score_s) sqrt(precisions[s]))
 *   out_lw[S * N]  may be NULL: row-major (S, N), the normalised log weights lw_s
 * tail_len: ceil(min(0.2 S, 3 sqrt(S / r_eff))) for a relative efficiency r_eff of the draws (1 for independent ones).
 * Everything is fp64; the sums over samples run in sample order, those over the grid in grid order: tile_rows / chunk_samples
 * (0: automatic) do not change a bit of the results. MFM_ERR_INVALID, before the device is used: what mfm_design_logdens*
 * refuses; more than 4096 samples; tail_len outside [0, S). N = 0 returns at once.                                            */
int mfm_design_loo_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                         const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                         int32_t chunk_samples, int32_t tail_len, double *out_elpd, double *out_k, double *out_lpd,
                         double *out_pit, double *out_lw);
int mfm_design_loo(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                   int64_t tile_rows, int32_t chunk_samples, int32_t tail_len, double *out_elpd, double *out_k,
                   double *out_lpd, double *out_pit, double *out_lw);
/* one row on the host, by the scalar pieces the kernel runs and in its summation orders (no device): log_lik[S], 1 <= S <= 4096,
 * tail_len in [0, S); out_lw[S] may be NULL                                                                                  */
int mfm_psis_row(int32_t S, int32_t tail_len, const double *log_lik, double *out_elpd, double *out_k, double *out_lw);

/* ---- chain diagnostics over the kept samples (csrc/mfm_ess.hpp) ------------------------------------------------
 * Per design row t, the split R-hat, the effective sample sizes and the Monte Carlo error of a per-sample value over the S
 * samples in their order, after Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021): the sequence is split into two halves
 * of floor(S / 2) draws, E(x) is Geyer's estimate over the halves' biased autocovariances as Stan runs it, Z(x) the rank-normalised
 * sequence (ties share the average rank).
 *   kind 0: the prediction value v_s, mode_or_task 0 the score, 1 Phi(score), 2 the expected class index under cutpoints[S][n_cut];
 *           y and precisions are NULL. out0 rhat = max(R of Z(v), R of Z(|v - median v|)), out1 ess_bulk = ess of Z(v), out2
 *           ess_mean = ess of v, out3 mcse_mean = sd(v, ddof = 1) / sqrt(ess_mean).
 *   kind 1: the likelihood u_s = exp(l_s - max_s l_s) with l_s, mode_or_task = task, y and the constants exactly as
 *           mfm_design_logdens* takes and checks them. out0 rhat and out1 ess_bulk of u as above, out2 r_eff = ess of u / S, out3
 *           mcse_lpd = sd(u, ddof = 1) / (mean(u) sqrt(ess of u)).
 * All four are NaN for S < 8, for a row with a non-finite value (an l of -inf under every sample) and where the halves do not
 * vary. Everything is fp64; the sums over samples run in sample order and those over lags in lag order: tile_rows /
 * chunk_samples (0: automatic) do not change a bit of the results. MFM_ERR_INVALID, before the device is used: a bad kind or
 * mode; for kind 1 what mfm_design_logdens* refuses; for kind 0 precisions given, cutpoints missing, non-finite or not ascending
 * for mode 2 or given otherwise; a missing output; negative tiling overrides; more than 4096 samples. N = 0 returns at once.   */
int mfm_design_ess_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t kind, int32_t mode_or_task,
                         const double *y, const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                         int32_t chunk_samples, double *out0, double *out1, double *out2, double *out3);
int mfm_design_ess(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t kind, int32_t mode_or_task, const double *y, const double *precisions, int32_t n_cut,
                   const double *cutpoints, int64_t tile_rows, int32_t chunk_samples, double *out0, double *out1, double *out2,
                   double *out3);
/* E(x) of one sequence on the host, by the scalar pieces the kernel runs and in its summation orders (no device): x[S],
 * 1 <= S <= 4096; NaN for S < 8 and where the halves do not vary                                                              */
int mfm_ess_row(int32_t S, const double *x, double *out_ess, double *out_rhat);
/* Several chains. The S samples are n_chains chains of L = S / n_chains draws each, chain after chain. Every chain is split as the
 * one chain above is, n = L / 2: sequence 2m is the samples [mL, mL + n), sequence 2m + 1 the samples [mL + L - n, mL + L), and E
 * compares the C = 2 n_chains sequences: A(t) is the mean of their autocovariances, V = A(0) + the variance (ddof = 1) of their
 * means, ess = C n / tau. Ranks, the median, the mean and the standard deviation are taken over all S samples. n_chains = 1 is
 * the entries above, bit for bit (they forward here). NaN where a chain has fewer than 8 draws. MFM_ERR_INVALID, before the
 * device is used, beyond what the entries above refuse: n_chains < 1, n_chains > 32, S not a multiple of n_chains.             */
int mfm_design_ess_chains_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t n_chains, int32_t kind,
                                int32_t mode_or_task, const double *y, const double *precisions, int32_t n_cut,
                                const double *cutpoints, int64_t tile_rows, int32_t chunk_samples, double *out0, double *out1,
                                double *out2, double *out3);
int mfm_design_ess_chains(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                          int32_t n_chains, int32_t kind, int32_t mode_or_task, const double *y, const double *precisions,
                          int32_t n_cut, const double *cutpoints, int64_t tile_rows, int32_t chunk_samples, double *out0,
                          double *out1, double *out2, double *out3);
int mfm_ess_row_chains(int32_t S, int32_t n_chains, const double *x, double *out_ess, double *out_rhat);
/* The three refusals of a chain count alone (no device; the message in mfm_global_error), and the largest count taken (32)    */
int mfm_ess_check_chains(int32_t n_samples, int32_t n_chains);
int32_t mfm_ess_max_chains(void);
/* out[j] = Phi^-1((1 + j / 2 - 3 / 8) / (S + 1 / 4)), j = 0 .. 2S - 2: the rank-normalised value of the average rank 1 + j / 2 */
int mfm_rank_z_table(int32_t S, double *out);

/* ---- continuous ranked probability score over the kept samples (csrc/mfm_crps.hpp) ----------------------------
 * Per design row t with observed target y[t], over the samples of mfm_design_summary*, the energy form
 * CRPS = E|Y - y| - E|Y - Y'| / 2 of the posterior predictive distribution of y (Y, Y' independent draws of it):
 *   task 0 (regression)      Y ~ (1 / S) sum_s N(score_s, 1 / precisions[s]); with A(m, v) = m erf(m h) + g exp(-(m h)^2),
 *                            h = 1 / sqrt(2 v), g = sqrt(2 v / pi):  accuracy = (1 / S) sum_s A(y - score_s, v_s),
 *                            spread = (1 / S^2) sum_s [sum_{t < s} A(score_s - score_t, v_s + v_t) + g(2 v_s) / 2]
 *   task 1 (probit), task 2 (ordered probit)   Y the class index 0 .. n_cut (task 1: one cutpoint 0, y in {0, 1}); per cut j
 *                            d_j = mean_s Phi(cut_sj - score_s) if y > j, else mean_s Phi(score_s - cut_sj):
 *                            accuracy = sum_j d_j, spread = sum_j d_j (1 - d_j), crps = sum_j d_j^2 (Brier / ranked probability score)
 *   out_crps[N]      accuracy - spread (task 0), sum_j d_j^2 (tasks 1, 2); >= 0
 *   out_accuracy[N]  E|Y - y|;   out_spread[N]  E|Y - Y'| / 2
 * Everything is fp64; the sums over t < s run in sample order into one sum per s, those in s order, the sums over samples of
 * tasks 1 and 2 in sample order and over cuts in cut order: tile_rows / chunk_samples (0: automatic) do not change a bit of the
 * results. MFM_ERR_INVALID, before the device is used: what mfm_design_logdens* refuses (the three outputs in the place of its
 * three), and for task 0 more than 1024 samples (S (S + 1) / 2 pair terms per row). Tasks 1 and 2 have no sample limit. N = 0
 * returns at once. The upload rule of the host flavour is that of mfm_design_summary.                                        */
int mfm_design_crps_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                          const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                          int32_t chunk_samples, double *out_crps, double *out_accuracy, double *out_spread);
int mfm_design_crps(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                    int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                    int64_t tile_rows, int32_t chunk_samples, double *out_crps, double *out_accuracy, double *out_spread);
/* one row on the host, by the functions the kernels run and in their summation orders (no device): scores[S], S >= 1 (task 0:
 * S <= 1024), precisions[S] (task 0, else NULL), cutpoints[S * n_cut] (task 2, else NULL and n_cut 0);
 * out[3] = (crps, accuracy, spread)                                                                                          */
int mfm_crps_row(int32_t task, int32_t S, double y, const double *scores, const double *precisions, int32_t n_cut,
                 const double *cutpoints, double *out);

/* ---- the score taken apart by field, over the kept samples (csrc/mfm_contrib.hpp) -------------------------------
 * field_of[n_field_of] gives every column of the flat design (main columns, then the relation blocks') a field in [0, n_fields).
 * For a design row x and a sample s:  p_g[k] = sum_{j in g} x_j V_s[k, j],  q_g = sum_{j in g} x_j^2 sum_k V_s[k, j]^2,
 *   lin_g = sum_{j in g} x_j w_s[j],   I_gg = (sum_k p_g[k]^2 - q_g) / 2,   I_gh = sum_k p_g[k] p_h[k]  (g < h),
 *   score_s = w0_s + sum_g lin_g + sum_{g <= h} I_gh.
 * Per row and component the mean and the population standard deviation over the samples (a streaming mean and M2 in sample
 * order), components along the first axis:
 *   out_bias[2]                          mean and standard deviation of w0
 *   out_linear, out_linear_std           (F, N)
 *   out_interaction, out_interaction_std (P, N), P = F (F + 1) / 2, pair (g, h), g <= h, at row g F - g (g - 1) / 2 + (h - g)
 * Everything is fp64 without atomics; tile_rows / chunk_samples (0: automatic) do not change a bit of the results. Relation blocks
 * are read in place. MFM_ERR_INVALID, before the device is used: n_fields outside [1, 16], n_field_of different from the design's
 * number of columns, a field outside [0, n_fields), a negative tiling override, a missing output; then the checks of the sample
 * source. N = 0 returns after out_bias is written. The upload rule of the host flavour is that of mfm_design_summary.       */
int mfm_design_contrib_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t n_fields, const int32_t *field_of,
                             int64_t n_field_of, int64_t tile_rows, int32_t chunk_samples, double *out_bias, double *out_linear,
                             double *out_linear_std, double *out_interaction, double *out_interaction_std);
int mfm_design_contrib(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t n_fields, const int32_t *field_of, int64_t n_field_of, int64_t tile_rows, int32_t chunk_samples,
                       double *out_bias, double *out_linear, double *out_linear_std, double *out_interaction,
                       double *out_interaction_std);
/* one row on the host, by the functions the kernel runs and in its orders (no device): the row's n entries (idx, val) in the flat
 * design of D columns, in the order main matrix, then block by block; ws[S * D], Vs[S * rank * D] (factor-major per sample);
 * out_mean[F + P], out_std[F + P]: the linear terms, then the interactions                                                    */
int mfm_contrib_row(int32_t n, const int32_t *idx, const double *val, int64_t D, int32_t rank, int32_t S, const double *ws,
                    const double *Vs, int32_t n_fields, const int32_t *field_of, int64_t n_field_of, double *out_mean, double *out_std);

/* ---- leave-one-out predictions over the kept samples (csrc/mfm_loo_pred.hpp) -------------------------------------
 * The weights w_s = exp(lw_s) of mfm_design_loo* applied to what the samples predict. The arguments up to tail_len are those of
 * mfm_design_loo*, out_k[N] is its k^ bit for bit. A row with an l_s of -inf has NaN everywhere and k^ = +inf.
 * mfm_design_loo_summary*: of the value v_s that mfm_design_summary* summarises (task 0 the score, task 1 Phi(score), task 2 the
 * expected class index under the sample's cutpoints)
 *   out_mean[N]   sum_s w_s v_s;   out_std[N]  sqrt(sum_s w_s (v_s - mean)^2)
 *   out_q[n_q * N]  row-major (n_q, N), n_q <= 32, probs[n_q] in [0, 1] in any order: with the samples ordered by (v_s, s) and c_i the
 *                 running sum of the weights in that order, v_(0) if c_0 >= p, else for the first i with c_i >= p
 *                 v_(i-1) + (v_(i) - v_(i-1)) clamp((p - c_(i-1)) / (c_i - c_(i-1)), 0, 1), else v_(S-1)  (the loo package's E_loo)
 *   out_std_y[N]  task 0 only, may be NULL: sqrt(std^2 + sum_s w_s / precisions[s])
 *   out_ess[N]    1 / sum_s w_s^2
 * mfm_design_loo_crps*: mfm_design_crps* with the predictive distribution reweighted (A, g as there)
 *   task 0        accuracy = sum_s w_s A(y - score_s, v_s), spread = sum_s w_s [sum_{u < s} w_u A(score_s - score_u, v_s + v_u)
 *                 + w_s g(2 v_s) / 2], crps = accuracy - spread; at most 1024 samples
 *   tasks 1, 2    d_j = sum_s w_s Phi(+-(cut_sj - score_s)), accuracy = sum_j d_j, spread = sum_j d_j (1 - d_j), crps = sum_j d_j^2
 * Everything is fp64 and summed in sample order (pair sums in u order, then in s order; cuts in cut order): tile_rows /
 * chunk_samples do not change a bit. MFM_ERR_INVALID, before the device is used: what mfm_design_loo* refuses, the quantile
 * refusals of mfm_design_summary*, for the task-0 CRPS more than 1024 samples. N = 0 returns at once.                          */
int mfm_design_loo_summary_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                                 const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                                 int32_t chunk_samples, int32_t tail_len, int32_t n_q, const double *probs, double *out_mean,
                                 double *out_std, double *out_q, double *out_std_y, double *out_ess, double *out_k);
int mfm_design_loo_summary(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                           int64_t tile_rows, int32_t chunk_samples, int32_t tail_len, int32_t n_q, const double *probs,
                           double *out_mean, double *out_std, double *out_q, double *out_std_y, double *out_ess, double *out_k);
int mfm_design_loo_crps_store(mfm_design *d, mfm_store *st, int32_t first, int32_t count, int32_t task, const double *y,
                              const double *precisions, int32_t n_cut, const double *cutpoints, int64_t tile_rows,
                              int32_t chunk_samples, int32_t tail_len, double *out_crps, double *out_accuracy, double *out_spread,
                              double *out_k);
int mfm_design_loo_crps(mfm_design *d, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                        int32_t task, const double *y, const double *precisions, int32_t n_cut, const double *cutpoints,
                        int64_t tile_rows, int32_t chunk_samples, int32_t tail_len, double *out_crps, double *out_accuracy,
                        double *out_spread, double *out_k);
/* one row on the host, by the scalar pieces the kernels run and in their summation orders (no device). Summary: values[S] (v_s) and
 * log_weights[S], 1 <= S <= 4096; inv_alpha[S] and out_std_y together or both NULL; out_q[n_q] in the order of probs. CRPS:
 * scores[S], log_weights[S], the constants of mfm_crps_row; out[3] = (crps, accuracy, spread)                                   */
int mfm_loo_summary_row(int32_t S, const double *values, const double *log_weights, const double *inv_alpha, int32_t n_q,
                        const double *probs, double *out_mean, double *out_std, double *out_q, double *out_std_y, double *out_ess);
int mfm_loo_crps_row(int32_t task, int32_t S, double y, const double *scores, const double *log_weights, const double *precisions,
                     int32_t n_cut, const double *cutpoints, double *out);

/* ---- query x candidate scoring with fused top-k (csrc/mfm_pairs.hip) -----------------------------------------
 * Two sparse sides in the model's full feature space, X_query (U, D) and X_cand (I, D), each optionally with relation blocks
 * (below); pair (u, i) is the design row X_query[u] + X_cand[i]. No column may be stored in both sides (MFM_ERR_INVALID "X_query and X_cand share column
 * ..."): the score then splits into per-side terms and one dense contraction, which runs on the fp64 MFMA. The arguments are
 * checked before the device is looked for, so a machine without a GPU gets MFM_ERR_INVALID for bad ones and MFM_ERR_DEVICE
 * otherwise. The handle's last error: the one of the pairs entry points (NULL: of the last failed create of this thread).
 *   mode 0: value(u, i) = mean_s score_s(u, i);  mode 1: mean_s Phi(score_s(u, i))   (as the prediction entry points above)
 *   mode 2: ordered probit, mean_s sum_j Phi(score_s(u, i) - cut_s[j]) = the posterior mean of the expected class index
 *           sum_c c p_c; needs mfm_pairs_set_cutpoints with the call's sample count and n_cut >= 1, else MFM_ERR_INVALID.
 *   add_block: side (0 query, 1 candidates) row r additionally holds row o2b[r] of a CSR block (block_rows, width) with
 *           block-local column indices, placed at columns [col_offset, col_offset + width) of the feature space. Blocks of a side
 *           are applied in the order they were added. MFM_ERR_INVALID, with a message naming the offender, for a bad side, an
 *           o2b entry outside [0, block_rows), a malformed CSR, col_offset + width > D, and a stored column (referenced by a
 *           side row or not) that the other side stores in its main matrix or in an earlier block ("X_query and X_cand share
 *           column j", j in model coordinates) or that this side already stores.
 *   scores: out[U * I] row-major = value(u, i).
 *   topk:   per query row the k (1 <= k <= 256) candidates of largest value, ordered by (value descending, candidate index
 *           ascending); idx[U * k], score[U * k] row-major, a tail of idx -1 / score -inf where fewer than k candidates remain.
 *           The pairs stored in the exclusion pattern (CSR pattern (U, I), NULL indptr: none) are left out.
 *   *_store: over samples [first, first + count) of a device store read in place; the others take host samples laid out as
 *           for the host-sample prediction entry point (w0s[S], ws[S * D], Vs[S * D * K], each V column-major (D, K)).
 * Memory: the candidate side's embedding (I x S x K doubles, padded) is resident for the call and refused when it exceeds
 * MFM_STORE_MAX_FRACTION of the free device memory; the queries are walked in chunks whose scratch stays under the scratch
 * bound (256 MB by default, never less than one 64-row tile). Every block's table (block_rows x S x (K + 2) doubles, padded,
 * both sides) is built once per call and counts as resident next to the candidate embedding.                              */
typedef struct mfm_pairs mfm_pairs;
int mfm_pairs_create(int device, int64_t D, int64_t U, const int64_t *q_indptr, const int32_t *q_indices, const double *q_data,
                     int64_t I, const int64_t *c_indptr, const int32_t *c_indices, const double *c_data, mfm_pairs **out);
void mfm_pairs_destroy(mfm_pairs *p);
const char *mfm_pairs_last_error(const mfm_pairs *p);
int mfm_pairs_set_exclude(mfm_pairs *p, const int64_t *indptr, const int32_t *indices);
int mfm_pairs_set_scratch_bound(mfm_pairs *p, int64_t bytes);
int mfm_pairs_add_block(mfm_pairs *p, int32_t side /*0 query, 1 cand*/, int64_t col_offset, int64_t width, int64_t block_rows,
                        const int64_t *o2b /*[U] or [I]*/, const int64_t *indptr, const int32_t *indices, const double *data);
int mfm_pairs_set_cutpoints(mfm_pairs *p, int32_t n_samples, int32_t n_cut, const double *cutpoints /*[n_samples][n_cut]*/);
int mfm_pairs_scores_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, double *out);
int mfm_pairs_topk_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int64_t *idx,
                         double *score);
int mfm_pairs_scores(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     int32_t mode, double *out);
int mfm_pairs_topk(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t mode, int32_t k, int64_t *idx, double *score);

/* ---- ranking by an upper confidence bound (csrc/mfm_pairs_ucb.hpp) ---------------------------------------------
 * The same pairs, sides, blocks, exclusions, sample views and memory rule, but the spread over the samples is kept. With v_s(u, i)
 * the per-sample value of the mode (0: score_s, 1: Phi(score_s), 2: sum_j Phi(score_s - cut_s[j])):
 *   mean = (sum_s v_s) / S,   std = the population standard deviation (ddof 0) of the v_s,   value = mean + beta * std,
 * the moments by Welford's recurrence in sample order (S = 1 and bitwise-equal v_s give std == 0.0 exactly).
 *   moments:  mean[U * I], std[U * I] row-major, every pair.
 *   topk_ucb: per query row the k (1 <= k <= 256) candidates of largest value under the order of topk; idx, value, mean,
 *             std are [U * k] row-major. mean and std are recomputed for the selected pairs after the merge, with the factors
 *             summed in another association than the selecting kernel's, so value and mean + beta * std agree within rounding,
 *             not bit for bit. Tail: idx -1, value -inf, mean and std NaN. beta: any finite number (negative: a lower bound).
 * A non-finite beta and k outside [1, 256] are MFM_ERR_INVALID before any launch.                                          */
int mfm_pairs_moments_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, double *mean, double *std);
int mfm_pairs_moments(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                      int32_t mode, double *mean, double *std);
int mfm_pairs_topk_ucb_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *std);
int mfm_pairs_topk_ucb(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t mode, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *std);

/* ---- ranks of given pairs among all candidates (csrc/mfm_pairs_rank.hpp) -----------------------------------------
 * The same sides, blocks, exclusions, sample views and memory rule. set_targets: a CSR pattern (U, I) of the pairs to rank, the
 * columns of a row sorted and unique, at most 64 per row, none of them excluded (checked against the exclusions whichever of the
 * two is set last); a violation is MFM_ERR_INVALID and the message names the query row and the candidate. A null indptr clears.
 *   rank: for the p-th stored target (u, i), rank_out[p] = the number of candidates j != i of query u that are not excluded and
 *         beat it under the order of topk (value descending, candidate index ascending) -- other targets of the row count --
 *         and value_out[p] = the pair's value, bit for bit what scores / topk give for it. Exact and independent of the
 *         chunking. Without targets or candidates nothing is written and nothing is launched.                              */
int mfm_pairs_set_targets(mfm_pairs *p, const int64_t *indptr, const int32_t *indices);
int mfm_pairs_rank_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int64_t *rank_out,
                         double *value_out);
int mfm_pairs_rank(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                   int32_t mode, int64_t *rank_out, double *value_out);

/* ---- ranking under each kept sample (csrc/mfm_pairs_samples.hpp) ----------------------------------------------------
 * The same sides, blocks, exclusions, sample views, order and memory rule, but the samples are not folded: with v_s(u, i) of the
 * section above, sample s ranks the candidates of query u by (v_s(u, i) descending, i ascending).
 *   topk_samples: row_sample == NULL: every sample's list, idx and value [count * U * k] row-major (sample, query, position).
 *             Otherwise row_sample[U] with entries in [0, count): only the list of query u under sample row_sample[u] (Thompson
 *             sampling when the entries are drawn uniformly), idx and value [U * k]; each query is contracted against one sample.
 *             An entry outside the range is MFM_ERR_INVALID and the message names the row. Tail: idx -1, value -inf.
 *             A list is bit for bit the topk of that one sample (the value of a pair under a sample is finished by shared code).
 *   topk_prob: per query the n_top (1 <= n_top <= 256) candidates that the most samples hold among their k best, ordered by
 *             (count descending, candidate index ascending), ties for the last place going to the smaller index;
 *             idx [U * n_top], prob [U * n_top] = count / count-of-samples, an fp64 division. Missing entries: idx -1, prob 0.0.
 *             The lists are counted on the device and never reach the host. count * k may not exceed MFM_PAIRS_VOTE_MAX (a
 *             query's votes are sorted in the device's local memory).
 * MFM_ERR_INVALID before any launch, with no output written: k outside [1, 256], n_top outside [1, 256], count * k over the vote's
 * limit, a bad row_sample entry, mode 2 without cutpoints. The query chunks take half the scratch bound; each chunk's work -- one
 * (sample, row tile) per workgroup -- is walked in slices whose per-stripe lists fit the rest (never less than one tile): results
 * do not depend on the bound.                                                                                                   */
#define MFM_PAIRS_VOTE_MAX 32768
int mfm_pairs_topk_samples_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k,
                                 const int32_t *row_sample, int64_t *idx, double *value);
int mfm_pairs_topk_samples(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t mode, int32_t k, const int32_t *row_sample, int64_t *idx, double *value);
int mfm_pairs_topk_prob_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t mode, int32_t k, int32_t n_top,
                              int64_t *idx, double *prob);
int mfm_pairs_topk_prob(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                        int32_t mode, int32_t k, int32_t n_top, int64_t *idx, double *prob);

/* ---- similar rows under each kept sample (csrc/mfm_pairs_sim.hpp) ----------------------------------------------------
 * "Which items are like this item": the geometry of the rows of V. For side rows a (query side) and b (candidate side), with
 * P_s[a, k] = sum_j V_s[k, j] a_j the embedding of a under kept sample s (relation blocks as above),
 *   metric MFM_PAIRS_SIM_COSINE: c_s(a, b) = (<P_s[a], P_s[b]> * r_s[a]) * r_s[b],  r = 1 / sqrt(sum_k P_k^2) with the squares summed
 *          in factor order, r = 0 where that sum is 0 (an empty row, rank 0, an all-zero embedding: the value is 0, not NaN). This holds for
 *          finite embeddings: where a row's sum of squares overflows, r is 0 too and the value may be NaN;
 *          the value is not clamped to [-1, 1].
 *   metric MFM_PAIRS_SIM_DOT:    r = 1, the inner product (for sides with disjoint columns the interaction part of the pair score).
 * The samples' factors differ by signs and rotations, so the cosine is formed under each sample and then summarised:
 *   mean = (sum_s c_s) / S,   std = the population standard deviation of the c_s (Welford's recurrence in sample order, as the
 *   moments above),   value = mean + beta * std.   w0, w, the cutpoints and the task play no part; w0s and ws are not read.
 *   create_sim: mfm_pairs_create without the check that the sides store disjoint columns (items against items share every column);
 *          add_block on such a handle still refuses a column its own side already stores. A similarity handle serves the four entry
 *          points below only: scores, topk, moments, topk_ucb, rank, topk_samples, topk_prob and the _vb entry points return
 *          MFM_ERR_INVALID on it, with a message that says so (their decomposition is wrong when columns are shared).
 *   sim:      mean[U * I], std[U * I] row-major, every pair; U * I > 2^24 is MFM_ERR_INVALID.
 *   topk_sim: per query row the k (1 <= k <= 256) candidates of largest value under the order of topk, the exclusion pattern left
 *          out; idx, value, mean, std [U * k] as topk_ucb returns them (mean and std recomputed for the selected pairs in another
 *          association: equal to the selecting kernel's within rounding, bit for bit on exact data). Tail: idx -1, value -inf, mean
 *          and std NaN.
 * Both work on either kind of handle, with the sample views, chunks, stripes and memory rule of the moments entry points.
 * MFM_ERR_INVALID before any launch: a metric outside {0, 1}, k outside [1, 256], a non-finite beta, the dense call's pair limit.  */
#define MFM_PAIRS_SIM_COSINE 0
#define MFM_PAIRS_SIM_DOT 1
int mfm_pairs_create_sim(int device, int64_t D, int64_t U, const int64_t *q_indptr, const int32_t *q_indices, const double *q_data,
                         int64_t I, const int64_t *c_indptr, const int32_t *c_indices, const double *c_data, mfm_pairs **out);
int mfm_pairs_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, double *mean, double *std);
int mfm_pairs_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs, int32_t metric,
                  double *mean, double *std);
int mfm_pairs_topk_sim_store(mfm_pairs *p, mfm_store *st, int32_t first, int32_t count, int32_t metric, int32_t k, double beta,
                             int64_t *idx, double *value, double *mean, double *std);
int mfm_pairs_topk_sim(mfm_pairs *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                       int32_t metric, int32_t k, double beta, int64_t *idx, double *value, double *mean, double *std);

/* ---- folding new one-hot features into the kept samples (csrc/mfm_foldin.hip) ----------------------------------
 * U new entities (users or items that were not in the training table), each a new one-hot column with value 1 in its own
 * observations. X (n, D) holds the CONTEXT of the n observations in the model's feature space (not the new column), y their
 * targets; the observations are grouped by entity: entity u owns rows [entity_offsets[u], entity_offsets[u + 1]), an entity may
 * own none. Under kept sample s the new column's parameters theta = (w_u, V_u1 .. V_uK) have the Gaussian posterior
 *   Lambda = diag(lambda_s) + alpha_s sum_i z_i z_i^T,  b = diag(lambda_s) mu_s + alpha_s sum_i z_i r_i,  theta_mean = Lambda^-1 b
 * with z_i = (1, q_s(x_i)), q_sk(x) = sum_j V_s[k, j] x_j and r_i = y_i - score_s(x_i); fit_linear = 0 drops the w_u component (the
 * written w_new is 0). alpha[S], mu[S][K + 1], lambda[S][K + 1]: per sample the noise precision and the prior mean / precision of
 * (w, V_1 .. V_K) -- component 0 is read only with fit_linear. draw = 0 writes the posterior mean; draw != 0 writes
 * theta_mean + L^-T eps (Lambda = L L^T), eps_j the Box-Muller value of counter word j >> 1 (r cos for even j, r sin for odd j) of
 * the per-row Philox stream keyed (seed, the fold-in draw tag, row = s U + u), j counting the components of theta. An entity without
 * observations gets the prior: mu bit for bit, or mu_j + eps_j / sqrt(lambda_j). Outputs: w_new[S][U], V_new[S][U][K].
 * The arguments are checked before the device is looked for (MFM_ERR_INVALID: a malformed CSR or offsets, a non-finite y or value;
 * per call: a rank above the limit returned by the max_rank entry point (64), a precision that is not positive and finite). A posterior
 * precision matrix that is not positive definite is MFM_ERR_INVALID from the call, never a NaN in the result.
 * A result does not depend on U, on the chunking or on the scratch bound (bytes of results per chunk of entities and samples; 256 MB
 * by default). *_store reads samples [first, first + count) of a device store in place; the other takes host samples laid out as
 * for the host-sample prediction entry point. The handle's last error: NULL for the last failed create of this thread.        */
typedef struct mfm_foldin mfm_foldin;
int mfm_foldin_create(int device, int64_t D, int64_t n, const int64_t *indptr, const int32_t *indices, const double *data,
                      const double *y, int64_t U, const int64_t *entity_offsets /*[U + 1]*/, int32_t fit_linear, mfm_foldin **out);
void mfm_foldin_destroy(mfm_foldin *p);
const char *mfm_foldin_last_error(const mfm_foldin *p);
int mfm_foldin_set_scratch_bound(mfm_foldin *p, int64_t bytes);
int mfm_foldin_max_rank(void);
int mfm_foldin_solve_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, const double *alpha, const double *mu,
                           const double *lambda, int32_t draw, uint64_t seed, double *w_new, double *V_new);
int mfm_foldin_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                     const double *alpha, const double *mu, const double *lambda, int32_t draw, uint64_t seed, double *w_new,
                     double *V_new);

/* ---- the same for the probit tasks: a short Albert-Chib chain per (entity, sample) (csrc/mfm_foldin_gibbs.hip) ----
 * The handle is mfm_foldin_create's; its y holds the labels: +-1 for the classifier (task 0), class indices in [0, n_class) for
 * ordered probit (task 1; cutpoints[S][n_class - 1], the group's cutpoints of every sample; NULL and n_class ignored for task 0).
 * Both tasks have noise precision 1, so Lambda = diag(lambda_s) + sum_i z_i z_i^T = U^T U is fixed. From theta^0 = mu, sweep
 * t = 0 .. T - 1, T = n_burn + n_inner: m_i = f_i + z_i^T theta^t; d_i a truncated standard normal (classifier: above -m_i for
 * y_i > 0, else below; ordered probit: between the cutpoints of the class, minus m_i) on the per-row Philox stream keyed (seed,
 * the fold-in latent tag + t, row = s n + i), i the grouped row and n the handle's row count; r_i = z_i^T theta^t + d_i;
 * b = lambda mu + sum_i z_i r_i; thetabar^{t+1} = Lambda^-1 b; theta^{t+1} = thetabar^{t+1} + U^-1 eps^t, eps^t_j as the closed
 * form's normals but on draw word (the fold-in draw tag + 1 + t). draw != 0 writes theta^T, a posterior draw given sample s;
 * draw = 0 writes the mean of thetabar^{t+1} over t >= n_burn. An entity without observations gets mu bit for bit, or
 * mu_j + eps^{T-1}_j / sqrt(lambda_j). fit_linear = 0 writes w_new = 0. Outputs: w_new[S][U], V_new[S][U][K].
 * MFM_ERR_INVALID before any launch: lambda not positive and finite, mu or a cutpoint not finite, cutpoints not non-decreasing, a
 * label that is not an integer in [0, n_class), n_inner < 1, n_burn < 0, T > 65535, a rank above the limit. A non-finite model
 * value is MFM_ERR_INVALID from the call and zeros in the result. A cell keeps n_u (M + 1) doubles of scratch; the call walks
 * entities, then samples, in chunks that stay under the handle's scratch bound, and a result does not depend on that.          */
int mfm_foldin_gibbs_solve_store(mfm_foldin *p, mfm_store *st, int32_t first, int32_t count, int32_t task, int32_t n_class,
                                 const double *cutpoints, const double *mu, const double *lambda, int32_t n_burn, int32_t n_inner,
                                 int32_t draw, uint64_t seed, double *w_new, double *V_new);
int mfm_foldin_gibbs_solve(mfm_foldin *p, int32_t rank, int32_t n_samples, const double *w0s, const double *ws, const double *Vs,
                           int32_t task, int32_t n_class, const double *cutpoints, const double *mu, const double *lambda,
                           int32_t n_burn, int32_t n_inner, int32_t draw, uint64_t seed, double *w_new, double *V_new);

/* FM::predict_score of the LIVE sample (the FM* handed to the per-iteration callback,
 * FMTrainer.hpp:78; utils/callbacks/libfm.py:85): scores design `d` with the (w0, w, V) currently
 * resident in training context `ctx` -- no download / upload of the model state. Same device only.  */
int mfm_design_score_ctx(mfm_design *d, mfm_ctx *ctx, double *out);

/* ---- test hooks: kernel-level access to the special functions / samplers of the classification and
 * ordered-probit tasks, so that parity tests can hold them against the reference's own code ----------- */
/* out[i] = the device erfcx(x[i]) used by mfm_oprobit_eval (reference: cpp_source/Faddeeva.cc erfcx, called from
 * OProbitSampler.hpp:111-236).                                                                           */
int mfm_test_erfcx(int device, const double *x, int64_t n, double *out);
/* n draws of the device truncated-normal samplers (util.hpp:15-78) with unit deviation: kind 0 = left
 * (z > lo, sample_truncated_normal_left), 1 = right (z < hi, :68-71), 2 = two-sided (lo < z < hi, :39-60). Draw i
 * uses the Philox stream keyed (seed, draw_index, row = i) -- the keying of mfm_update_e_classification.        */
int mfm_test_truncated_normal(int device, int32_t kind, double lo, double hi, uint64_t seed, uint64_t draw_index,
                              int64_t n, double *out);

/* ---- host-only helpers (no device needed; exercised by the CPU test-suite) -------------- */
/* Level schedule of the columns of a CSR matrix: level[j] = 0 if no earlier
 * column shares a row with column j, else 1 + max level of those columns. Returns the number
 * of levels in *n_levels.                                                                   */
int mfm_host_column_levels(int64_t n_rows, int64_t n_cols, const int64_t *indptr, const int32_t *indices,
                           int32_t *level, int32_t *n_levels);
/* The plan of the streamed block-feature sweep of a large relation block (FMTrainer.hpp:276-302, :419-470 as ONE pipelined launch,
 * csrc/mfm_chain_plan.hpp) for the chain over ALL n_cols columns of the block's CSC (colptr / rowidx / val: column j -> ascending block
 * rows), steps of cg columns, a window of lw steps, nb row ranges, slot reuse delay rd, at most cap LDS slots -- and an emulation of the
 * launch's data flow on the host (every actor on its own copy of what it can see, in the earliest order its flags allow) against the
 * plain sequential sweep: *max_rel_diff = the largest relative difference of coefficients / records (rounding level when the plan is
 * right). info[8]: built (0 / 1: the hot rows did not fit), slots, most entering / leaving rows of a step, cold entries, hot entries,
 * most hot entries of a column, steps.                                                                                          */
int mfm_cs_plan_selftest(int64_t n_rows, int32_t n_cols, const int64_t *colptr, const int32_t *rowidx, const double *val, int32_t cg,
                         int32_t lw, int32_t nb, int32_t rd, int32_t cap, double *max_rel_diff, int64_t *info);
/* The same planner as the launch takes it, for tests that must prove which of the kernel's paths a design reaches: the plan with
 * (cg, lw, nb, rd) as given and no slot cap. rec[MFM_CHAIN_STREAM_INFO_FIELDS]: one record of mfm_chain_stream_info (block and
 * launches 0); hot_per_col[n_cols] (may be NULL): hot entries of every column; *built: 1 when the kernel could launch the plan (the
 * walker's LDS and its staged entry lists hold it), else 0 -- the record then shows what it would have needed, and nothing is
 * emulated; *max_rel_diff as above.                                                                                             */
int mfm_cs_plan_probe(int64_t n_rows, int32_t n_cols, const int64_t *colptr, const int32_t *rowidx, const double *val, int32_t cg,
                      int32_t lw, int32_t nb, int32_t rd, int64_t *rec, int32_t *hot_per_col, int32_t *built, double *max_rel_diff);

/* ---- variational inference (csrc/mfm_vb.hip): the device steps of VariationalFMTrainer::update_all
 * (include/myfm/variational.hpp:192-217, BaseFMTrainer.hpp:135-152). An mfm_vb holds the table -- the main table with the
 * rows of its relation blocks appended (CSR, and CSC in a conflict-free level order of its columns) --, y, the group of
 * every feature, the model
 * (w0, w0_var, w, w_var, V, V_var; V / V_var column-major (D, K)) and the per-row residual e. It takes none of the Gibbs
 * context's fast paths and draws no random numbers: after the initial weights (drawn by the host) the iteration is
 * deterministic, and every sum has a fixed association, so a rerun is bit-identical. Per-group arrays are packed by "slot":
 * slot 0 is w, slot 1 + f is factor f, entry (slot s, group g) at [s * G + g].                                               */
typedef struct mfm_vb mfm_vb;
/* VariationalFMTrainer(X, relations, y, ...) (variational.hpp:180-185, BaseFMTrainer.hpp:58-105) in three calls: the (N, D0)
 * main table and y; each relation block (B rows, Db columns, original_to_block (N)), in order; then finalize with
 * group_index (D = D0 + the blocks' columns, values in [0, G)) and the rank. The blocks' rows are appended to the train
 * rows that map to them: the block caches of the reference (:388-447, :557-710, :728-827) are sums over those rows, so the
 * iteration is the same in exact arithmetic. A row that holds a column twice is refused (MFM_ERR_INVALID).              */
int mfm_vb_create(int device, int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices, const double *data,
                  const double *y, mfm_vb **out);
int mfm_vb_add_block(mfm_vb *v, int64_t B, int64_t Db, const int64_t *indptr, const int32_t *indices, const double *data,
                     const int64_t *original_to_block);
int mfm_vb_finalize(mfm_vb *v, const int32_t *group_index, int32_t G, int32_t rank);
/* Row-sharded mode, all before mfm_vb_finalize (the counterparts of mfm_set_stream, mfm_set_allreduce, mfm_set_shard,
 * mfm_comm_init, mfm_comm_stats, mfm_set_main_levels). The context holds rows [row_offset, row_offset + N) of n_total_rows
 * and a replica of the model; a context with a communicator runs every level of a sweep as statistics -> ONE all-reduce of
 * the level's sums -> apply, and all-reduces the four sums of mfm_vb_update_e as one buffer: (K + 1) * (non-empty levels) + 1
 * collectives per iteration. A world of 1 with a communicator takes the same path. With a shard declared mfm_vb_create's N may
 * be 0 (an empty shard takes part in every collective with zeros); otherwise mfm_vb_finalize refuses N < 1.
 * mfm_vb_set_stream: run on the caller's stream (a callback provider enqueues its all-reduce on it) instead of the context's
 * own; before mfm_vb_comm_init. mfm_vb_comm_init: RCCL called from this library on the context's stream, id128 from
 * mfm_comm_unique_id.
 * mfm_vb_set_levels: the level of every column of the GLOBAL expanded design (mfm_vb_design_levels on all rows). The ranks'
 * own schedules could differ and their collectives would not match, so a world of more than one rank must pass it;
 * mfm_vb_finalize uses it instead of computing its own and returns MFM_ERR_INVALID, having launched nothing, unless along every
 * local row the levels grow with the column index (so no two columns of one level share a row).
 * mfm_vb_design_levels: host only, no device: the expansion mfm_vb_finalize does (block k: block_rows[k] x block_cols[k] CSR and
 * its original_to_block (N)) and the levels of its D0 + sum block_cols columns into level_out.                              */
int mfm_vb_set_stream(mfm_vb *v, void *hip_stream);
int mfm_vb_set_allreduce(mfm_vb *v, int (*fn)(void *user, void *dev_buf, int64_t count), void *user);
int mfm_vb_set_shard(mfm_vb *v, int32_t rank, int32_t world, int64_t n_total_rows, int64_t row_offset);
int mfm_vb_comm_init(mfm_vb *v, const void *id128, int32_t rank, int32_t world);
int mfm_vb_comm_stats(const mfm_vb *v, int64_t *calls, int64_t *doubles);
int mfm_vb_set_levels(mfm_vb *v, const int32_t *level, int64_t D);
int mfm_vb_design_levels(int64_t N, int64_t D0, const int64_t *indptr, const int32_t *indices, const double *data,
                         int32_t n_blocks, const int64_t *block_rows, const int64_t *block_cols,
                         const int64_t *const *block_indptr, const int32_t *const *block_indices,
                         const double *const *block_data, const int64_t *const *block_maps, int32_t *level_out,
                         int32_t *n_levels);
void mfm_vb_destroy(mfm_vb *v);
const char *mfm_vb_last_error(const mfm_vb *v); /* (NULL: the error of the last failed mfm_vb_create of this thread) */
/* levels of the column schedule, kernel launches of one iteration (row-sharded: two per level) */
int mfm_vb_plan_info(const mfm_vb *v, int64_t *n_levels, int64_t *n_launches_per_iteration);
/* the model (VariationalFM, variational.hpp:64-103); NULL array pointers are skipped */
int mfm_vb_set_state(mfm_vb *v, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                     const double *V_var);
int mfm_vb_get_state(mfm_vb *v, double *w0, double *w0_var, double *w, double *w_var, double *V, double *V_var);
/* update_w0 (variational.hpp:348-361): the scalars only; the host shifts e with mfm_vb_shift_e */
int mfm_vb_set_w0(mfm_vb *v, double w0, double w0_var);
/* update_e_and_var (variational.hpp:715-833) and the residual: mode 0 e -= y (initialize_e :234-241, update_e for regression
 * :839-840), mode 1 e -= E[z] of the truncated normal (classification, :841-856). out4: sum e, sum e^2, e_var_sum (with
 * N * w0_var), sum over rows of lnZ + (E[z] - score)^2 / 2 (0 in mode 0). Row-sharded: the sums over all ranks' rows, with
 * n_total_rows * w0_var added once after the all-reduce; e is the local rows'.                                              */
int mfm_vb_update_e(mfm_vb *v, int32_t mode, double *out4);
int mfm_vb_shift_e(mfm_vb *v, double delta); /* e += delta (update_w0 :358) */
int mfm_vb_get_e(mfm_vb *v, double *e);
/* the per-row cache of the factor last swept by mfm_vb_sweep_V: q, x2s, x3sv (NULL skips) */
int mfm_vb_get_cache(mfm_vb *v, double *q, double *x2s, double *x3sv);
/* fit_linear == false: w = w_var = 0 without touching e (variational.hpp:364-367); the caller then sweeps anyway */
int mfm_vb_zero_w(mfm_vb *v);
/* update_w, main table (variational.hpp:368-386): lambda_w, mu_w (G) */
int mfm_vb_sweep_w(mfm_vb *v, double alpha, const double *lambda_w, const double *mu_w);
/* update_V, main table (variational.hpp:450-554) for factors [f_begin, f_end): lambda_V, mu_V column-major (G, K) */
int mfm_vb_sweep_V(mfm_vb *v, int32_t f_begin, int32_t f_end, double alpha, const double *lambda_V, const double *mu_V);
/* per slot s in [s_begin, s_end) and group g, with mu / mu_var packed by slot ((K + 1) * G each): out[((s - s_begin) * G + g)
 * * 3 + k] = sum theta, sum ((theta - mu)^2 + mu_var + var), sum log var over the group's features (update_lambda_generic
 * :269-295, update_mu_generic :298-318, the weight terms of the ELBO :872-917).                                            */
int mfm_vb_group_stats(mfm_vb *v, int32_t s_begin, int32_t s_end, const double *mu, const double *mu_var, double *out);
int mfm_vb_synchronize(mfm_vb *v);
/* mean_var_truncated_normal_left (right = 0) / _right (right = 1) (util.hpp:80-115) on the host, by the same code the
 * classification residual of mfm_vb_update_e runs on the device: out3 = mean, variance, log Z                              */
int mfm_vb_truncated_normal(int32_t right, double mu, double *out3);

/* ---- analytic score moments of a variational model (csrc/mfm_vbmoments.hpp, csrc/mfm_pairs_vb.hpp) -------------------
 * The model is the mean-field Gaussian posterior w0 ~ N(w0, w0_var), w ~ N(w[D], w_var[D]), V ~ N(V, V_var), V and V_var column-major
 * (D, K), all host arrays. Under it the FM score of a row has the closed-form mean (the mean model's score) and variance
 *   w0_var + sum x^2 w_var + sum_k [ M^2 A - 2 M B + C + (A^2 - E) / 2 ]_k  + extra_var
 * with M = sum x m, A = sum x^2 s, B = sum x^3 s m, C = sum x^4 s m^2, E = sum x^4 s^2 over the row's entries (relation blocks
 * included, never expanded). extra_var >= 0 is added as it is (1 / alpha: the predictive variance of a regression target).
 * mfm_design_moments_vb: out_mean[N] is bit for bit the score mfm_design_predict gives for the mean model on a design without
 *   relation blocks; out_std[N] = sqrt(max(variance, 0)); want_prob != 0 also writes out_prob[N] = Phi(mean / sqrt(1 + variance)),
 *   the probit link integrated over a Gaussian with these two moments (out_prob may be NULL otherwise). tile_rows forces the rows per
 *   launch (0: automatic); the results do not depend on it. rank <= 512.
 * mfm_pairs_moments_vb: mean[U * I] and std[U * I] of the score of every pair of an mfm_pairs handle (its sides, blocks, scratch
 *   bound and query chunking); mean is bit for bit mfm_pairs_scores' (mode 0) for the mean model as its one sample.
 * mfm_pairs_topk_bound_vb: per query row the k candidates of largest mean + beta * std that are not excluded, in mfm_pairs_topk's order
 *   and with mfm_pairs_topk_ucb's outputs and tail (idx -1, value -inf, mean and std NaN); mean and std are recomputed for the selected
 *   pairs in another association than the selecting kernel's, so value and mean + beta * std agree within rounding.
 * NULL outputs, a negative rank, negative or non-finite variances, a non-finite beta and k outside [1, 256] are MFM_ERR_INVALID before
 * any launch; a NULL handle is MFM_ERR_INVALID with the message under mfm_design_last_error(NULL) / mfm_pairs_last_error(NULL).   */
int mfm_design_moments_vb(mfm_design *d, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                          const double *V_var, double extra_var, int32_t want_prob, int64_t tile_rows, double *out_mean,
                          double *out_std, double *out_prob);
int mfm_pairs_moments_vb(mfm_pairs *p, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                         const double *V_var, double extra_var, double *mean, double *std);
int mfm_pairs_topk_bound_vb(mfm_pairs *p, int32_t rank, double w0, double w0_var, const double *w, const double *w_var, const double *V,
                            const double *V_var, double extra_var, int32_t k, double beta, int64_t *idx, double *value, double *mean,
                            double *std);

#ifdef __cplusplus
}
#endif
#endif /* MYFM_HIP_H_ */
