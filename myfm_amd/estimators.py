"""sklearn-style estimators over the MI355X backend: the MyFMRegressor / MyFMClassifier /
MyFMOrderedProbit surface of the reference (src/myfm/base.py:70-399, src/myfm/gibbs.py:32-543),
written against ``myfm_amd._myfm``. Same constructor / fit / predict arguments, defaults and
error behaviour; numpy-2 safe.
"""
import os
from collections import OrderedDict, namedtuple
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
from scipy import sparse as sps
from scipy import special

from . import _myfm
from ._myfm import ConfigBuilder, RelationBlock, TaskType

REAL = np.float64


def std_cdf(x):
    """Standard normal CDF (base.py:41-43)."""
    return (1 + special.erf(np.asarray(x) * np.sqrt(0.5))) / 2


def check_data_consistency(X, X_rel) -> int:
    """Number of cases shared by X and the relation blocks (base.py:46-61)."""
    if X_rel:
        sizes = {rel.mapper_size for rel in X_rel}
        if len(sizes) > 1:
            raise ValueError("Inconsistent case size for X_rel.")
        n = sizes.pop()
        if X is not None and X.shape[0] != n:
            raise ValueError("X and X_rel have different shape.")
        return n
    if X is None:
        raise ValueError("At least X or X_rel must be provided.")
    return int(X.shape[0])


def _as_csr(X, n_rows) -> sps.csr_matrix:
    if X is None:
        return sps.csr_matrix((n_rows, 0), dtype=REAL)
    X = sps.csr_matrix(X)
    if X.dtype != REAL:
        X = X.astype(REAL)
    # canonical CSR is a precondition of the sampler (duplicates would change sum x^2)
    if not X.has_canonical_format:
        X = X.copy()
        X.sum_duplicates()
    return X


class _ProgressBar:
    """tqdm when available (base.py:303-312), silent otherwise."""

    def __init__(self, total):
        try:
            from tqdm import tqdm

            self.bar = tqdm(total=total)
        except Exception:  # pragma: no cover
            self.bar = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        if self.bar is not None:
            self.bar.close()

    def update(self, message, n=1):
        if self.bar is not None:
            if message is not None:
                self.bar.set_description(message)
            self.bar.update(n)


class _FMEstimatorBase:
    """What the Gibbs and the variational estimators share (base.py:70-323): arguments, fit's argument handling, prediction."""

    _task_type = TaskType.REGRESSION
    _variational = False  # MyFMVariationalBase: create_train_vfm, rows in the caller's order

    def __init__(
        self,
        rank: int,
        init_stdev: float = 0.1,
        random_seed: int = 42,
        alpha_0: float = 1.0,
        beta_0: float = 1.0,
        gamma_0: float = 1.0,
        mu_0: float = 0.0,
        reg_0: float = 1.0,
        fit_w0: bool = True,
        fit_linear: bool = True,
        exact_latent_draws: bool = True,
    ):
        # exact_latent_draws (not in the reference, which has one generator and nothing to choose). True (default): under the same
        # seed EVERY draw is the reference's own -- also the latent draws of MyFMClassifier / MyFMOrderedProbit, which the reference
        # makes row after row inside rejection loops on its one std::mt19937: they are evaluated in parallel on the device from that
        # same stream (csrc/mfm_latent.hip), in the caller's row order whatever order the device paths keep the rows in. False: the
        # latent draws come from per-row Philox streams instead (same law, other numbers: posterior means agree with the reference's
        # chain only statistically) -- 1.15x faster at 5 10^7 rows, 5x at 10^7 rows of a two-field table. Regression chains are the
        # reference's draw for draw either way. Row-sharded fits always use the per-row streams.
        self.exact_latent_draws = bool(exact_latent_draws)
        self.rank = rank
        self.init_stdev = init_stdev
        self.random_seed = random_seed
        self.alpha_0 = alpha_0
        self.beta_0 = beta_0
        self.gamma_0 = gamma_0
        self.mu_0 = mu_0
        self.reg_0 = reg_0
        self.fit_w0 = fit_w0
        self.fit_linear = fit_linear
        self.predictor_ = None
        self.history_ = None
        self.n_groups_: Optional[int] = None

    def __str__(self) -> str:
        return (
            "{}(init_stdev={}, alpha_0={}, beta_0={}, gamma_0={}, mu_0={}, reg_0={})".format(
                self.__class__.__name__, self.init_stdev, self.alpha_0, self.beta_0, self.gamma_0, self.mu_0, self.reg_0
            )
        )

    # ---- hooks specialised per task ------------------------------------------------------------
    def _process_y(self, y):
        return np.asarray(y).astype(REAL)

    def _status_report(self, fm, hyper) -> str:
        raise NotImplementedError

    def _prepare_prediction_for_test(self, fm, X, X_rel):
        raise NotImplementedError

    def _measure_score(self, prediction, y) -> Dict[str, float]:
        raise NotImplementedError

    # ---- fitting -----------------------------------------------------------------------------------
    def _default_callback(self, freq, do_test, X_test, X_rel_test, y_test):
        def callback(i, fm, hyper, history):
            if i % freq:
                return False, None
            msg = self._status_report(fm, hyper)
            if do_test:
                pred = self._prepare_prediction_for_test(fm, X_test, X_rel_test)
                for key, metric in self._measure_score(pred, y_test).items():
                    msg += " {}_this: {:.2f}".format(key, metric)
            return False, msg

        return callback

    def _fit(
        self,
        X,
        y,
        X_rel=[],
        X_test=None,
        y_test=None,
        X_rel_test=[],
        n_iter: int = 100,
        n_kept_samples: Optional[int] = None,
        grouping: Optional[List[int]] = None,
        group_shapes: Optional[List[int]] = None,
        callback=None,
        config_builder: Optional[ConfigBuilder] = None,
        callback_default_freq: int = 10,
    ) -> None:
        if config_builder is None:
            config_builder = ConfigBuilder()
        y = np.asarray(y)
        train_size = check_data_consistency(X, X_rel)
        X = _as_csr(X, train_size)
        assert X.shape[0] == y.shape[0]
        dim_all = X.shape[1] + sum(rel.feature_size for rel in X_rel)

        if n_kept_samples is None:
            n_kept_samples = min(max(n_iter - 5, 5), n_iter)  # base.py:238-239
        else:
            assert n_iter >= n_kept_samples

        for key in ("alpha_0", "beta_0", "gamma_0", "mu_0", "reg_0", "fit_w0", "fit_linear"):
            getattr(config_builder, "set_" + key)(getattr(self, key))

        if group_shapes is not None and grouping is None:
            grouping = [g for g, size in enumerate(group_shapes) for _ in range(size)]
        if grouping is None:
            self.n_groups_ = 1
            self.grouping_ = None  # (one field)
            config_builder.set_identical_groups(dim_all)
        else:
            assert dim_all == len(grouping)
            self.n_groups_ = len(set(grouping))
            self.grouping_ = np.asarray([int(g) for g in grouping], dtype=np.int32)
            config_builder.set_group_index([int(g) for g in grouping])

        if X_test is not None or X_rel_test:
            if y_test is None:
                raise RuntimeError("Must specify both (X_test or X_rel_test) and y_test.")
            test_size = check_data_consistency(X_test, X_rel_test)
            assert test_size == np.asarray(y_test).shape[0]
            X_test = _as_csr(X_test, test_size)
            do_test = True
        elif y_test is not None:
            raise RuntimeError("Must specify both (X_test or X_rel_test) and y_test.")
        else:
            do_test = False

        config_builder.set_n_iter(n_iter).set_n_kept_samples(n_kept_samples)
        y = self._process_y(y)
        # The sampler does not depend on the order of the training rows (every conditional is a sum over rows), the
        # device path does: a table sorted by its first one-hot field runs the fused passes. Rows that
        # arrive in another order are sorted by the first stored column here, together with y and the relation maps.
        perm = None if self._variational else _device_row_order(X)
        if perm is not None:
            ptr, idx, val = _myfm.permute_csr_rows(X.indptr, X.indices, X.data, perm)
            X = sps.csr_matrix((val, idx, ptr), shape=X.shape)
            y = np.asarray(y)[perm]
            X_rel = [RelationBlock(r.original_to_block_array[perm], r.data) for r in X_rel]
            if self._task_type != TaskType.REGRESSION:
                # the latent draws are made in the CALLER's row order (FMTrainer.hpp:500, OProbitSampler.hpp:243): the sorted
                # table's row that is the caller's row i
                inv = np.empty(perm.shape[0], dtype=np.int64)
                inv[perm] = np.arange(perm.shape[0], dtype=np.int64)
                if self._task_type == TaskType.ORDERED:
                    config_builder.set_cutpoint_groups([(int(np.asarray(y).max()) + 1, inv)])
                else:
                    config_builder.set_latent_row_order(inv)
        config_builder.set_task_type(self._task_type)
        if not self._variational:
            config_builder.set_exact_latent_draws(self.exact_latent_draws and not os.environ.get("MYFM_AMD_PHILOX_LATENT"))
        config = config_builder.build()

        default_callback = callback is None
        if default_callback:
            callback = self._default_callback(callback_default_freq, do_test, X_test, X_rel_test, y_test)

        with _ProgressBar(n_iter) as bar:
            seen = [0]

            def wrapped(i, fm, hyper, history) -> bool:
                should_stop, message = callback(i, fm, hyper, history)
                bar.update(message, i + 1 - seen[0])
                seen[0] = i + 1
                return bool(should_stop)

            if default_callback:
                # the default callback only acts every `callback_default_freq` iterations (base.py:179-205): the trainer calls into
                # Python on those (and the last one) only -- the iterations in between never leave the C++ loop
                wrapped.myfm_every = max(1, int(callback_default_freq))

            from . import distributed as _dist

            if self._variational and _dist.active():
                # row-sharded: the same data on every rank, each trains on its contiguous slice of the rows as they come
                # (VB does not re-sort them), with the level schedule of the whole expanded design
                rank, world = _dist.rank_world()
                n = X.shape[0]
                lo, hi = _dist.row_range(n, rank, world)
                levels = _myfm.vb_column_levels(X, list(X_rel))
                rel_l = [RelationBlock(r.original_to_block_array[lo:hi], r.data) for r in X_rel]
                y_l = np.ascontiguousarray(np.asarray(y, dtype=REAL)[lo:hi])
                kw = {k: v for k, v in _dist.comm_kwargs().items() if k != "peer_connect"}  # (a Gibbs path)
                self.predictor_, self.history_ = _myfm.create_train_vfm_sharded(
                    self.rank, self.init_stdev, X[lo:hi], rel_l, y_l, self.random_seed, config, wrapped, rank, world, n, lo,
                    levels, **kw)
            elif self._variational:
                self.predictor_, self.history_ = _myfm.create_train_vfm(
                    self.rank, self.init_stdev, X, list(X_rel), np.ascontiguousarray(y, dtype=REAL), self.random_seed, config,
                    wrapped)
            elif _dist.active():
                # row-sharded over the process group: same data on every rank, each trains on its slice
                from . import _capi

                rank, world = _dist.rank_world()
                n = X.shape[0]
                levels, _ = _capi.column_levels(X) if X.shape[1] else (np.zeros(0, np.int32), 0)
                if X.shape[1] and np.diff(X.indptr).min() >= 1:
                    cuts = _dist.shard_cuts(X.indices[X.indptr[:-1]], world)
                else:
                    cuts = [(n * r) // world for r in range(world + 1)]
                lo, hi = cuts[rank], cuts[rank + 1]
                # the latent draws of a shard come from per-row Philox streams, which need no caller's row order; the
                # cutpoint group lists LOCAL rows
                config_builder.set_latent_row_order(np.zeros(0, dtype=np.int64))
                if self._task_type == TaskType.ORDERED:
                    config_builder.set_cutpoint_groups([(int(np.asarray(y).max()) + 1, np.arange(hi - lo, dtype=np.int64))])
                config = config_builder.build()
                rel_l = [RelationBlock(r.original_to_block_array[lo:hi], r.data) for r in X_rel]
                y_l = np.ascontiguousarray(np.asarray(y, dtype=REAL)[lo:hi])
                self.predictor_, self.history_ = _myfm.create_train_fm_sharded(
                    self.rank, self.init_stdev, X[lo:hi], rel_l, y_l, self.random_seed, config, wrapped, rank, world, n, lo,
                    np.ascontiguousarray(levels, dtype=np.int32), **_dist.comm_kwargs())
            else:
                self.predictor_, self.history_ = _myfm.create_train_fm(
                    self.rank, self.init_stdev, X, list(X_rel), np.ascontiguousarray(y, dtype=REAL), self.random_seed, config,
                    wrapped)

    # ---- posterior access ---------------------------------------------------------------------------
    def _fetch_predictor(self):
        if self.predictor_ is None:
            raise RuntimeError("Predictor called before fit.")
        return self.predictor_

    def _predict_core(self, X, X_rel=[], n_workers: Optional[int] = None):
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        if n_workers is None:
            return predictor.predict(X, list(X_rel))
        return predictor.predict_parallel(X, list(X_rel), n_workers)


PredictiveSummary = namedtuple("PredictiveSummary", ["mean", "std", "quantiles"])
PREDICT_DIST_MAX_QUANTILES = 32
FOLD_IN_MAX_RANK = 64  # fold_in factors a (rank + 1)^2 matrix per (entity, sample) in the device's local memory (csrc/mfm_foldin.hpp)
PREDICT_DIST_MAX_SAMPLES = 4096  # with a non-empty `quantiles`: a row's values are sorted in the device's local memory


def _checked_quantiles(quantiles):
    probs = np.asarray(quantiles, dtype=REAL)
    if probs.ndim != 1:
        raise ValueError("quantiles must be a 1-D sequence of probabilities")
    if probs.shape[0] > PREDICT_DIST_MAX_QUANTILES:
        raise ValueError("at most %d quantiles per call" % PREDICT_DIST_MAX_QUANTILES)
    if not np.all((probs >= 0.0) & (probs <= 1.0)):  # (NaN fails both comparisons)
        raise ValueError("quantiles must lie in [0, 1]")
    return probs


def _check_sample_limit(probs, n_samples):
    if probs.shape[0] > 0 and n_samples > PREDICT_DIST_MAX_SAMPLES:
        raise ValueError("quantiles are computed over at most %d kept samples, this model keeps %d (mean and std have no "
                         "limit: pass quantiles=())" % (PREDICT_DIST_MAX_SAMPLES, n_samples))


def _kept_precisions(est, n_samples, what):
    """the noise precision alpha_s of every kept sample: the last n_samples entries of history_.hypers"""
    hypers = None if est.history_ is None else est.history_.hypers
    if hypers is None or len(hypers) < n_samples:
        raise RuntimeError("%s needs history_ with the noise precision of every kept sample" % what)
    return np.asarray([h.alpha for h in hypers[len(hypers) - n_samples:]], dtype=REAL)


class _PredictiveDistMixin:
    """Posterior predictive summaries of a fitted Gibbs regressor / classifier. MyFMOrderedProbit and the
    variational estimators have no predict_dist (for ordered probit see predict_proba_dist / predict_expected_dist; the variational
    estimators give the analytic moments of their posterior instead, predict_moments). Row-sharded
    operation is not covered: the model is replicated, so each rank may call predict_dist on its own rows."""

    def predict_dist(self, X, X_rel=[], quantiles=(0.05, 0.5, 0.95), noise=False):
        """PredictiveSummary(mean, std, quantiles) per test row over the S kept samples, computed on the device in one pass
        over the test rows. The per-sample value v_s is the sample's score for a regressor and Phi(score) for a classifier.

        mean (N,): what predict / predict_proba return, bit for bit. std (N,): population standard deviation (ddof = 0) of
        the v_s. quantiles (Q, N): np.quantile(v, quantiles, axis=0) under the default "linear" rule, from exactly sorted
        values; `quantiles` may be empty (at most 32 entries in [0, 1]; S <= 4096 unless it is empty).

        noise=True (regressor only) describes y itself, the equal-weight mixture of N(score_s, 1 / alpha_s) with alpha_s
        the noise precision of the iteration that produced sample s (the last S entries of history_.hypers): the mean is
        unchanged, std is sqrt(var_s(score) + mean_s(1 / alpha_s)) and the quantiles are those of the mixture, solved per
        row on the device; they must then lie strictly inside (0, 1).

        The arguments are checked on the host before the device is touched."""
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        probs = _checked_quantiles(quantiles)
        n_samples = len(predictor.samples)
        precisions = None
        if noise:
            if self._task_type != TaskType.REGRESSION:
                raise ValueError("noise=True describes a regression target: it is not available on a classifier")
            if np.any((probs <= 0.0) | (probs >= 1.0)):
                raise ValueError("with noise=True the quantiles must lie strictly inside (0, 1)")
            precisions = _kept_precisions(self, n_samples, "noise=True")
        _check_sample_limit(probs, n_samples)
        return PredictiveSummary(*predictor.predict_dist(X, list(X_rel), probs, precisions))


PointwiseDensity = namedtuple("PointwiseDensity", ["lpd", "log_lik_mean", "log_lik_var", "pit", "log_lik"])


class _LogDensityMixin:
    """How probable were the observed targets under the posterior: the pointwise log predictive density of a fitted Gibbs
    regressor, classifier or ordered probit. The variational estimators keep no samples (their posterior is one Gaussian,
    summarised analytically by predict_moments) and have no such method. Row-sharded operation is not covered: the model is replicated, so each rank may call it on its own rows."""

    def predict_log_density(self, X, y, X_rel=[], pointwise=False):
        """PointwiseDensity(lpd, log_lik_mean, log_lik_var, pit, log_lik) per test row over the S kept samples, computed on the
        device in one pass over the rows. With l_s = log p(y | sample s) -- the normal density with that sample's noise precision
        (the last S entries of history_.hypers, as predict_dist(noise=True) takes them), log Phi(+-score) for a classifier, the log
        of the class interval's probability under that sample's cutpoints for ordered probit --

        lpd (N,): logsumexp_s l_s - log S, the log pointwise predictive density. log_lik_mean (N,): mean_s l_s. log_lik_var (N,):
        the sample variance (ddof = 1) of the l_s, WAIC's penalty (exactly 0 for one kept sample). pit (N,), regressor only (else
        None): the predictive CDF at y, mean_s Phi((y - score_s) sqrt(alpha_s)), uniform on [0, 1] for a calibrated model.
        log_lik (S, N), only with pointwise=True (else None and nothing of that size exists on the host): the l_s themselves,
        for arviz or one's own estimators (PSIS-LOO itself runs on the device: predict_loo). The tails are evaluated without forming Phi: finite wherever the scores are.

        y (N,) as fit takes it: real targets, 0 / 1 or bool labels, integer classes in [0, n_class) (MyFMOrderedProbit also takes
        cutpoint_index, the cutpoint group). See myfm_amd.utils.evaluation for waic, log_score and pit_histogram.

        The arguments are checked on the host before the device is touched."""
        return self._predict_log_density(X, y, X_rel, pointwise, None)

    def _predict_log_density(self, X, y, X_rel, pointwise, cutpoint_index):
        predictor, args = self._log_density_args(X, y, X_rel, cutpoint_index, "predict_log_density")
        return PointwiseDensity(*predictor.predict_log_density(*args, bool(pointwise)))

    def _log_density_args(self, X, y, X_rel, cutpoint_index, what):
        """(predictor, (X, X_rel, y, task, precisions, cutpoints)): what predict_log_density and predict_loo hand to the predictor"""
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        y = np.asarray(y)
        if y.ndim != 1 or y.shape[0] != n:
            raise ValueError("y must hold one value per row: expected shape (%d,), got %s" % (n, y.shape))
        if y.dtype.kind not in "buif" or not np.all(np.isfinite(y)):
            raise ValueError("y must be finite")
        if self._task_type == TaskType.ORDERED and y.shape[0] and y.min() < 0:
            raise ValueError("ordered-probit labels must be integers in [0, n_class)")
        y = self._process_y(y) if y.shape[0] else y.astype(REAL)
        precisions = cutpoints = None
        if self._task_type == TaskType.REGRESSION:
            precisions = _kept_precisions(self, len(predictor.samples), what)
        elif self._task_type == TaskType.CLASSIFICATION:
            y = (y + 1) / 2  # (fit's -1 / +1 back to the 0 / 1 the device call takes)
        else:
            if isinstance(cutpoint_index, bool) or not isinstance(cutpoint_index, (int, np.integer)):
                raise ValueError("cutpoint_index must be an integer")
            cutpoints = int(cutpoint_index)
        return predictor, (X, list(X_rel), np.ascontiguousarray(y, dtype=REAL), int(self._task_type), precisions, cutpoints)


LooDensity = namedtuple("LooDensity", ["elpd_loo", "pareto_k", "lpd", "loo_pit", "log_weights"])
LooPredictive = namedtuple("LooPredictive", ["mean", "std", "quantiles", "std_y", "ess", "pareto_k"])
LooCrps = namedtuple("LooCrps", ["crps", "accuracy", "spread", "pareto_k"])
PREDICT_LOO_MAX_SAMPLES = PREDICT_DIST_MAX_SAMPLES  # a row's importance ratios are sorted in the device's local memory


class _LooMixin(_LogDensityMixin):
    """Pareto-smoothed importance-sampling leave-one-out of a fitted Gibbs regressor, classifier or ordered probit (DESIGN
    4.9.3), after Vehtari, Gelman and Gabry (2017) and Vehtari et al. (2024). Limits: one tail length for all rows (r_eff is one
    number, given or with "auto" the mean of the rows' estimates from the chain: no per-row tail length); no moment matching or
    refit for rows with a large k; at most 4096 kept samples; no variational estimator; not row-sharded (the model is replicated:
    each rank may call it on its own rows). predict_loo_dist and predict_loo_crps apply the same weights to what
    the samples predict; their further limits: at most 32 quantiles, a regressor CRPS over at most 1024 kept samples, and one k
    per row -- no separate Pareto fit per summarised function."""

    def predict_loo(self, X, y, X_rel=[], log_weights=False, r_eff=1.0):
        """LooDensity(elpd_loo, pareto_k, lpd, loo_pit, log_weights) per row over the S kept samples, computed on the device in one
        pass over the rows. The leave-one-out reading holds when X, y are rows the model was fitted on: the importance ratios
        1 / p(y | sample s) then turn the posterior into the posterior without that row. For other rows the numbers are still
        computed, but they estimate nothing.

        With l_s = log p(y | sample s) as predict_log_density takes it, the largest M = ceil(min(0.2 S, 3 sqrt(S / r_eff))) ratios
        are replaced by the quantiles of a generalized Pareto distribution fitted to them and the weights w_s are normalised.
        elpd_loo (N,): log sum_s w_s p(y | sample s). pareto_k (N,): the shape k of the fit, the diagnostic (see
        myfm_amd.utils.evaluation.loo for the threshold); +inf where no fit was made: M < 5 (S < 25 at r_eff = 1), a tail whose lower
        quarter equals the cutoff, or a sample under which y has density 0 (then elpd_loo = -inf). lpd (N,): bit for bit
        predict_log_density(X, y).lpd, so that p_loo = lpd - elpd_loo needs no second call. loo_pit (N,), regressor only (else
        None): sum_s w_s Phi((y - score_s) sqrt(alpha_s)); pit_histogram(result.loo_pit) takes it. log_weights (S, N), only with
        log_weights=True (else None and nothing of that size exists on the host): log w_s.

        r_eff: the relative efficiency of the draws, one finite positive number (1: independent draws), used for M alone; or "auto":
        the mean of the finite per-row r_eff of likelihood_diagnostics on the same rows (1 if none is finite), one more pass over
        the rows. At most 4096 kept samples. X, y, X_rel (MyFMOrderedProbit: cutpoint_index) as predict_log_density takes and checks them; all
        arguments are checked on the host before the device is touched."""
        return self._predict_loo(X, y, X_rel, log_weights, r_eff, None)

    def _predict_loo(self, X, y, X_rel, log_weights, r_eff, cutpoint_index):
        if not isinstance(log_weights, (bool, np.bool_)):
            raise ValueError("log_weights must be a bool")
        predictor, args, r_eff = self._loo_args(X, y, X_rel, r_eff, cutpoint_index, "predict_loo")
        return LooDensity(*predictor.predict_loo(*args, bool(log_weights), r_eff))

    def _loo_args(self, X, y, X_rel, r_eff, cutpoint_index, what, max_samples=None):
        """(predictor, the arguments of _log_density_args, r_eff as one number): what every leave-one-out method checks, in
        predict_loo's order, and "auto" resolved. max_samples: (limit, message) of a method with a limit of its own."""
        auto = isinstance(r_eff, str) and r_eff == "auto"
        if not auto and (isinstance(r_eff, (bool, np.bool_)) or not isinstance(r_eff, (int, float, np.integer, np.floating))
                         or not np.isfinite(r_eff) or not r_eff > 0):
            raise ValueError("r_eff must be one finite positive number, or \"auto\"")
        predictor, args = self._log_density_args(X, y, X_rel, cutpoint_index, what)
        n_samples = len(predictor.samples)
        if n_samples > PREDICT_LOO_MAX_SAMPLES:
            raise ValueError("leave-one-out weights are computed over at most %d kept samples, this model keeps %d"
                             % (PREDICT_LOO_MAX_SAMPLES, n_samples))
        if max_samples is not None and n_samples > max_samples[0]:
            raise ValueError(max_samples[1] % (max_samples[0], n_samples))
        if auto:  # the chain's own estimate, one number for all rows (as arviz hands PSIS one)
            per_row = np.asarray(predictor.likelihood_ess(*args, n_chains=int(getattr(self, "n_chains_", 1)))[2])
            r_eff = float(np.nanmean(per_row)) if np.any(np.isfinite(per_row)) else 1.0  # (a row is finite or NaN)
        return predictor, args, float(r_eff)

    def predict_loo_dist(self, X, y, X_rel=[], quantiles=(0.05, 0.5, 0.95), r_eff=1.0):
        """LooPredictive(mean, std, quantiles, std_y, ess, pareto_k) per row: what the model predicts for a row it was fitted on
        when that row is left out, computed on the device in one pass over the rows. The per-sample value v_s is
        that of predict_dist / predict_expected_dist -- the score for a regressor, Phi(score) for a classifier, the expected class
        index for ordered probit -- and the weights are w_s = exp(log_weights) of predict_loo, which never leave the device.

        mean (N,): sum_s w_s v_s. std (N,): sqrt(sum_s w_s (v_s - mean)^2), the mean taken first. quantiles (Q, N): the
        inverse-CDF rule of the loo package's E_loo -- with the samples ordered by (v_s, s) and c_i the running sum of the weights
        in that order, the quantile at p is v_(0) if c_0 >= p; else, for the first i with c_i >= p, v_(i-1) + (v_(i) - v_(i-1))
        (p - c_(i-1)) / (c_i - c_(i-1)); v_(S-1) if rounding leaves no such i. With equal weights this is not np.quantile's
        "linear" rule (which predict_dist follows): it inverts the step function of the weights and interpolates inside a step.
        std_y (N,), regressor only (else None): sqrt(std^2 + sum_s w_s / alpha_s), the leave-one-out predictive standard deviation
        of y itself, what a standardised leave-one-out residual divides by. ess (N,): 1 / sum_s w_s^2, Kish's effective number of
        weights. pareto_k (N,): predict_loo's, bit for bit. A row whose y has density 0 under some sample has NaN everywhere and
        pareto_k = +inf. See myfm_amd.utils.evaluation.loo_residuals.

        Limits: at most 32 quantiles (`quantiles` may be empty); at most 4096 kept samples; one k per row, that of the weights --
        no separate Pareto fit per summarised function, which E_loo makes for h r. r_eff as predict_loo takes it. X, y, X_rel
        (MyFMOrderedProbit: cutpoint_index) as predict_log_density takes and checks them; all arguments are checked on the host
        before the device is touched."""
        return self._predict_loo_dist(X, y, X_rel, quantiles, r_eff, None)

    def _predict_loo_dist(self, X, y, X_rel, quantiles, r_eff, cutpoint_index):
        probs = _checked_quantiles(quantiles)
        predictor, args, r_eff = self._loo_args(X, y, X_rel, r_eff, cutpoint_index, "predict_loo_dist")
        return LooPredictive(*predictor.predict_loo_dist(*args, probs, r_eff))

    def predict_loo_crps(self, X, y, X_rel=[], r_eff=1.0):
        """LooCrps(crps, accuracy, spread, pareto_k) per row: predict_crps with the predictive distribution reweighted by the
        leave-one-out weights w_s of predict_loo, on the device in one pass over the rows. Regressor: the mixture
        sum_s w_s N(score_s, 1 / alpha_s), accuracy = sum_s w_s A(y - score_s, v_s), spread = sum_s w_s [sum_{u < s} w_u
        A(score_s - score_u, v_s + v_u) + w_s g(2 v_s) / 2], crps = accuracy - spread; at most 1024 kept samples. Classifier and
        ordered probit: d_j = sum_s w_s Phi(+-(cut_sj - score_s)) in the place of predict_crps' mean, crps = sum_j d_j^2. With
        equal weights it is predict_crps. pareto_k (N,): predict_loo's, bit for bit; a row whose y has density 0 under some sample
        has NaN scores. myfm_amd.utils.evaluation.crps_summary takes the result as it takes predict_crps'.

        r_eff as predict_loo takes it; X, y, X_rel (MyFMOrderedProbit: cutpoint_index) as predict_log_density takes and checks
        them; all arguments are checked on the host before the device is touched."""
        return self._predict_loo_crps(X, y, X_rel, r_eff, None)

    def _predict_loo_crps(self, X, y, X_rel, r_eff, cutpoint_index):
        limit = None
        if self._task_type == TaskType.REGRESSION:
            limit = (PREDICT_CRPS_MAX_SAMPLES, "a regression CRPS is computed over at most %d kept samples, this model keeps %d")
        predictor, args, r_eff = self._loo_args(X, y, X_rel, r_eff, cutpoint_index, "predict_loo_crps", limit)
        return LooCrps(*predictor.predict_loo_crps(*args, r_eff))


CrpsScore = namedtuple("CrpsScore", ["crps", "accuracy", "spread"])
PREDICT_CRPS_MAX_SAMPLES = 1024  # regressor: a row costs S (S + 1) / 2 pair terms, the pair constants S (S + 1) doubles


class _CrpsMixin(_LogDensityMixin):
    """The continuous ranked probability score of a fitted Gibbs regressor, classifier or ordered probit: the
    proper scoring rule in the units of y, which reduces to the absolute error for a point forecast and which no single row
    dominates as it can the log score. Limits: a regressor with at most 1024 kept samples (the leave-one-out weighted
    form is predict_loo_crps); no variational estimator; one cutpoint group per call; not row-sharded (the model is replicated: each rank may call it on its
    own rows)."""

    def predict_crps(self, X, y, X_rel=[]):
        """CrpsScore(crps, accuracy, spread) per test row over the S kept samples, computed on the device in one pass over the
        rows: CRPS = E|Y - y| - E|Y - Y'| / 2 with Y, Y' independent draws of the posterior predictive distribution of y.

        Regressor: that distribution is the mixture mean_s N(score_s, 1 / alpha_s) of predict_dist(noise=True) (the noise
        precisions are the last S entries of history_.hypers), and both expectations have a closed form in erf and exp (Grimit
        et al. 2006) with S (S + 1) / 2 pair terms per row; at most 1024 kept samples. Classifier and ordered probit: Y is the
        class index, crps = sum_j (P(Y <= j) - 1[y <= j])^2 with P the posterior mean class probabilities: the Brier score of
        predict_proba for a classifier, the ranked probability score for ordered probit.

        accuracy (N,): E|Y - y|. spread (N,): E|Y - Y'| / 2. crps (N,): their difference, >= 0, smaller is better; for the
        discrete tasks summed directly and not as the difference. See myfm_amd.utils.evaluation.crps_summary.

        X, y, X_rel (MyFMOrderedProbit: cutpoint_index) as predict_log_density takes and checks them; all arguments are checked
        on the host before the device is touched."""
        return self._predict_crps(X, y, X_rel, None)

    def _predict_crps(self, X, y, X_rel, cutpoint_index):
        predictor, args = self._log_density_args(X, y, X_rel, cutpoint_index, "predict_crps")
        n_samples = len(predictor.samples)
        if self._task_type == TaskType.REGRESSION and n_samples > PREDICT_CRPS_MAX_SAMPLES:
            raise ValueError("a regression CRPS is computed over at most %d kept samples, this model keeps %d"
                             % (PREDICT_CRPS_MAX_SAMPLES, n_samples))
        return CrpsScore(*predictor.predict_crps(*args))


ScoreContributions = namedtuple("ScoreContributions", ["bias", "bias_std", "linear", "linear_std", "interaction", "interaction_std", "pairs"])
CONTRIB_MAX_FIELDS = 16  # a lane group of the device pass keeps the moments of all F + F (F + 1) / 2 components in registers


def _contribution_fields(est, D, grouping, group_shapes):
    """(F, field_of int32 (D,)) of a predict_contributions call: the arguments as fit takes them, or the fit's own grouping_"""
    if grouping is not None and group_shapes is not None:
        raise ValueError("give grouping or group_shapes, not both")
    F = None
    if group_shapes is not None:
        shapes = [int(v) for v in group_shapes]
        if any(v < 0 for v in shapes):
            raise ValueError("group_shapes must hold non-negative sizes")
        F = len(shapes)
        if not 1 <= F <= CONTRIB_MAX_FIELDS:
            raise ValueError("predict_contributions serves 1 to %d fields, got %d" % (CONTRIB_MAX_FIELDS, F))
        grouping = np.repeat(np.arange(F, dtype=np.int64), shapes)
    elif grouping is None:
        if not hasattr(est, "grouping_"):
            raise ValueError("this model does not record the grouping of its fit (it has no grouping_, as a model pickled by an "
                             "earlier version): pass grouping or group_shapes")
        grouping = np.zeros(D, dtype=np.int64) if est.grouping_ is None else est.grouping_
    g = np.asarray(grouping)
    if g.ndim != 1 or g.shape[0] != D:
        raise ValueError("the grouping must hold one field per column: %d expected, got shape %s" % (D, g.shape))
    if D and not np.issubdtype(g.dtype, np.integer):
        raise ValueError("the grouping must hold integers")
    if D and g.min() < 0:
        raise ValueError("the grouping holds a negative field")
    if F is None:
        F = int(g.max()) + 1 if D else 1
    if not 1 <= F <= CONTRIB_MAX_FIELDS:
        raise ValueError("predict_contributions serves 1 to %d fields, got %d" % (CONTRIB_MAX_FIELDS, F))
    return F, np.ascontiguousarray(g, dtype=np.int32)


class _ContributionsMixin:
    """The score of a fitted Gibbs regressor, classifier or ordered probit taken apart by field: which fields, and
    which pairs of fields, carry the prediction for a row. The inner products of the fields' embeddings are formed under every kept
    sample and summarised afterwards -- they are invariant to the signs, permutations and rotations that differ between the
    samples' factors, which an average of V is not. Limits: at most 16 fields; no variational estimator; not row-sharded."""

    def predict_contributions(self, X, X_rel=[], grouping=None, group_shapes=None):
        """ScoreContributions(bias, bias_std, linear, linear_std, interaction, interaction_std, pairs) of the rows of X over the S
        kept samples, computed on the device in one pass over the rows.

        With the columns of the flat design (X's, then the relation blocks') assigned to F fields, the score of a row under one
        sample is w0 + sum_g lin_g + sum_{g <= h} I_gh: lin_g the field's linear term, I_gh (g < h) the inner product of the two
        fields' embeddings p_g = sum_{j in g} x_j V[j], and I_gg the interactions inside field g (zero for a one-hot field).
        linear, linear_std (F, N) and interaction, interaction_std (P, N), P = F (F + 1) / 2: per row the mean and the population
        standard deviation of every component over the kept samples; row p of the interactions is the pair pairs[p] = (g, h);
        bias, bias_std: those of w0. All values are on the SCORE scale for every task: for a classifier and an ordered probit
        that is the probit's latent scale, not a probability. bias + linear.sum(0) + interaction.sum(0) is the posterior mean
        score (myfm_amd.utils.evaluation.contribution_total; see also contribution_matrix and contribution_summary).

        grouping (one field id in [0, F) per column) or group_shapes as fit takes them, not both; with neither the grouping of
        the fit (grouping_; None there: one field) is used -- a model without grouping_, as one pickled by an earlier version,
        must be given one. All arguments are checked on the host before the device is touched."""
        predictor = self._fetch_predictor()
        F, field_of = _contribution_fields(self, int(predictor.feature_size), grouping, group_shapes)
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        res = predictor.predict_contributions(X, list(X_rel), F, field_of)
        pairs = np.asarray([(g, h) for g in range(F) for h in range(g, F)], dtype=np.int64).reshape(-1, 2)
        return ScoreContributions(*res, pairs)


ChainDiagnostics = namedtuple("ChainDiagnostics", ["rhat", "ess_bulk", "ess_mean", "mcse_mean"])
LikelihoodDiagnostics = namedtuple("LikelihoodDiagnostics", ["r_eff", "rhat", "ess_bulk", "mcse_lpd"])


class _DiagnosticsMixin(_LogDensityMixin):
    """Have the kept samples mixed, and how many independent draws are they worth: per-row split R-hat, effective sample sizes and
    Monte Carlo errors of a fitted Gibbs regressor, classifier or ordered probit over the S kept samples in their order (DESIGN
    4.9.4), after Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021). The factors themselves are not identified (sign and
    rotation), so what is diagnosed are the identified per-row quantities every other summary is a Monte Carlo estimate of. One fit
    is one chain: the two halves of the kept samples stand in for two chains. A model that combine_chains or fit_chains made of M
    fits (n_chains_ = M) is M chains: every chain is split in two and the 2M halves are compared, which also sees chains that sit in
    different modes. Limits: no tail-ESS; at most 4096 kept samples in all and at most 32 chains of equal length; no variational
    estimator (one sample); not row-sharded (the model is replicated: each rank may call it on its own rows)."""

    def _n_chains(self):
        return int(getattr(self, "n_chains_", 1))

    def predict_diagnostics(self, X, X_rel=[]):
        """ChainDiagnostics(rhat, ess_bulk, ess_mean, mcse_mean) per row, computed on the device in one pass over the rows, of the
        per-sample value v_s that predict_dist summarises: the score for a regressor, Phi(score) for a classifier (for
        MyFMOrderedProbit the expected class index under cutpoint group `cutpoint_index`).

        rhat (N,): the larger of the split R-hat of the rank-normalised values and of the rank-normalised |v - median v|; above
        1.01 the halves of the chain disagree. ess_bulk (N,): the effective sample size of the rank-normalised values, behind the
        quantiles. ess_mean (N,): that of the values themselves, behind the mean; mcse_mean (N,) = sd(v, ddof = 1) / sqrt(ess_mean)
        is the Monte Carlo standard error of predict_dist's mean. All are NaN with fewer than 8 kept samples and for a row whose
        value does not vary; ess <= S log10(S). See myfm_amd.utils.evaluation.diagnostics_summary.

        The arguments are checked on the host before the device is touched."""
        return self._predict_diagnostics(X, X_rel, 0)

    def _predict_diagnostics(self, X, X_rel, cutpoint_index):
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        if isinstance(cutpoint_index, bool) or not isinstance(cutpoint_index, (int, np.integer)):
            raise ValueError("cutpoint_index must be an integer")
        self._check_diagnostics_limit(predictor)
        return ChainDiagnostics(*predictor.predict_ess(X, list(X_rel), int(cutpoint_index), n_chains=self._n_chains()))

    def likelihood_diagnostics(self, X, y, X_rel=[]):
        """LikelihoodDiagnostics(r_eff, rhat, ess_bulk, mcse_lpd) per row, computed on the device in one pass over the rows, of the
        per-sample likelihood u_s = p(y | sample s) (scaled by its maximum: nothing underflows) that predict_log_density averages
        and predict_loo weights by.

        r_eff (N,): the relative efficiency ess(u) / S, the loo package's relative_eff(exp(log_lik)); predict_loo(r_eff="auto")
        takes the mean of the finite ones. rhat, ess_bulk (N,): as predict_diagnostics, of u. mcse_lpd (N,) = sd(u, ddof = 1) /
        (mean(u) sqrt(ess(u))): the delta-method Monte Carlo standard error of lpd. NaN with fewer than 8 kept samples, for a row
        whose likelihood does not vary, and where y has density 0 under every sample.

        X, y, X_rel (MyFMOrderedProbit: cutpoint_index) as predict_log_density takes and checks them, on the host before the
        device is touched."""
        return self._likelihood_diagnostics(X, y, X_rel, None)

    def _likelihood_diagnostics(self, X, y, X_rel, cutpoint_index):
        predictor, args = self._log_density_args(X, y, X_rel, cutpoint_index, "likelihood_diagnostics")
        self._check_diagnostics_limit(predictor)
        rhat, ess_bulk, r_eff, mcse = predictor.likelihood_ess(*args, n_chains=self._n_chains())
        return LikelihoodDiagnostics(r_eff, rhat, ess_bulk, mcse)

    @staticmethod
    def _check_diagnostics_limit(predictor):
        n_samples = len(predictor.samples)
        if n_samples > PREDICT_LOO_MAX_SAMPLES:
            raise ValueError("chain diagnostics are computed over at most %d kept samples, this model keeps %d"
                             % (PREDICT_LOO_MAX_SAMPLES, n_samples))


def _ranked_args(Xq, Xc, k, exclude, beta=0.0):
    """The checks predict_topk and predict_topk_ucb share, in one order: (k int, beta float, exclude csr or None)."""
    if isinstance(k, bool) or int(k) != k:
        raise ValueError("k must be an integer in [1, 256]")
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not np.isfinite(beta):
        raise ValueError("beta must be a finite real number")
    if exclude is not None:
        exclude = sps.csr_matrix(exclude)
        if exclude.shape != (Xq.shape[0], Xc.shape[0]):
            raise ValueError("exclude must have shape (n_queries, n_candidates)")
    return int(k), float(beta), exclude


class _PairScoringMixin:
    """Ranking with a fitted model: scores of every (query row, candidate row) pair and the per-query top-k, computed on the
    device without materialising the pair rows. Regressors score the posterior-mean prediction, classifiers the
    mean over the samples of Phi(score) -- what predict / predict_proba return for the design row X_query[u] + X_cand[i]. The
    variational estimators have one sample, the mean model. MyFMOrderedProbit scores the posterior mean of the expected class
    index, sum_c c p_c per sample with that sample's cutpoints (group 0): predict_proba(pair rows) @ arange(n_class), from the
    device store and from host samples after unpickling alike.

    Without block arguments both sides are sparse matrices in the model's full feature space, (U, D) and (I, D) with D the fitted
    feature size. A model fitted with relation blocks has rows [X | B_0[idx_0] | B_1[idx_1] ...]; its sides are given as main
    matrices of the main width plus X_rel_query / X_rel_cand, each either empty (no blocks on that side) or a list with one entry
    per block position of the model: a RelationBlock whose mapper has one entry per row of that side, or None where the side
    holds nothing at that position (a user block is [ub, None] on the query side and [None, ib] on the candidate side). Main
    width + the blocks' widths must equal the feature size; a position that is None on both sides, two blocks of different
    width at one position and a mapper of the wrong size are ValueErrors. A block row's share of the embedding is computed once
    and gathered by the side rows that point at it.

    Either side may hold empty rows, multi-hot rows and non-unit values, but no column of the feature space may be stored in
    both, block columns included and referenced by a side row or not (ValueError naming the column in model coordinates).
    Not covered: row-sharded operation (the model is replicated, so each rank can call this on its own queries). The arguments
    are validated on the host before the device is touched."""

    def _pair_sides(self, X_query, X_cand, X_rel_query, X_rel_cand):
        predictor = self._fetch_predictor()
        if X_query is None or X_cand is None:
            raise ValueError("X_query and X_cand must be given.")
        rels = []
        for name, rel in (("X_rel_query", X_rel_query), ("X_rel_cand", X_rel_cand)):
            rel = [] if rel is None else list(rel)
            if any(r is not None and not isinstance(r, RelationBlock) for r in rel):
                raise ValueError("%s must hold RelationBlock or None entries" % name)
            rels.append(rel)
        return predictor, _as_csr(X_query, 0), _as_csr(X_cand, 0), rels[0], rels[1]

    def predict_pairs(self, X_query, X_cand, X_rel_query=[], X_rel_cand=[]):
        """(U, I) array of the value of every pair. U * I > 2^24 is refused (ValueError): use predict_topk."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        return predictor.predict_pairs(Xq, Xc, rq, rc)

    def predict_topk(self, X_query, X_cand, k: int, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Per query row the k candidates of largest value: (indices int64 (U, k), scores float64 (U, k)), each row ordered by
        (value descending, candidate index ascending). `exclude`: optional (U, I) scipy sparse matrix whose stored positions
        are pairs to leave out (the stored values are ignored). Where fewer than k candidates remain the tail is index -1,
        score -inf. 1 <= k <= 256, else ValueError."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, _, exclude = _ranked_args(Xq, Xc, k, exclude)
        return predictor.predict_topk(Xq, Xc, k, exclude, rq, rc)

    def predict_rank(self, X_query, X_cand, targets, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Where given pairs land in the ranking of all candidates of their query, computed on the device without the (U, I)
        matrix: the held-out evaluation of a recommender, with `targets` the held-out pairs and `exclude` the
        training pairs. `targets`: (U, I) scipy sparse pattern (stored values are ignored, stored zeros count); `exclude` as in
        predict_topk. Returns TargetRanks(rank int64 (nnz,), value float64 (nnz,), n_candidates int64 (U,)), rank and value in
        the order of the stored positions of `targets` as CSR with sorted indices:

        rank[p]: the number of non-excluded candidates of the pair's query that beat it under predict_topk's order (value
        descending, candidate index ascending). Other targets of the same row count, the target itself does not: rank 0 is the
        head of the predict_topk list. value[p]: the pair's value, bit for bit that of predict_pairs / predict_topk.
        n_candidates[u] = I - the number of excluded candidates of row u. myfm_amd.utils.ranking.ranking_metrics turns the
        result into MRR, AUC, NDCG@k and recall@k.

        The device takes at most 64 targets per row and call: rows with more are served by further calls over the rows that
        still have targets, and the ranks do not depend on that split. A target that is also excluded, a wrong shape and sides
        that share a column are ValueErrors, raised on the host before the device is touched."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        _, _, exclude = _ranked_args(Xq, Xc, 1, exclude)
        U, I = Xq.shape[0], Xc.shape[0]
        if targets is None or not sps.issparse(targets) or targets.shape != (U, I):
            raise ValueError("targets must be a scipy sparse matrix of shape (n_queries, n_candidates)")
        T = sps.csr_matrix(targets, copy=True)
        T.sum_duplicates()  # (sorts the indices too)
        n_candidates = np.full(U, I, dtype=np.int64)
        if exclude is not None:
            exclude = sps.csr_matrix(exclude, copy=True)
            exclude.sum_duplicates()
            n_candidates -= np.diff(exclude.indptr)
            pattern = lambda M: sps.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
            both = pattern(T).multiply(pattern(exclude)).tocoo()
            if both.nnz:
                raise ValueError("targets: the pair (query row %d, candidate %d) is also excluded" % (both.row[0], both.col[0]))
        rank, value = np.empty(T.nnz, dtype=np.int64), np.empty(T.nnz)
        per_row = np.diff(T.indptr)
        for lo in range(0, int(per_row.max()) if U else 0, _RANK_TARGETS_PER_CALL):
            rows = np.flatnonzero(per_row > lo)
            n = np.minimum(per_row[rows] - lo, _RANK_TARGETS_PER_CALL)
            # entry p of this call's pattern is stored target `at[p]` of T
            ptr = np.concatenate(([0], np.cumsum(n)))
            at = np.repeat(T.indptr[rows] + lo - ptr[:-1], n) + np.arange(ptr[-1])
            part = sps.csr_matrix((np.ones(at.size), T.indices[at], ptr), shape=(rows.size, I))
            whole = rows.size == U
            sub = lambda r: None if r is None else RelationBlock(np.asarray(r.original_to_block_array)[rows], r.data)
            rank[at], value[at] = predictor.predict_rank(
                Xq if whole else Xq[rows], Xc, part, exclude if whole or exclude is None else exclude[rows],
                rq if whole else [sub(r) for r in rq], rc)
        if per_row.size == 0 or per_row.max() == 0:
            # nothing to rank: the arguments are still checked by the binding, which launches nothing
            predictor.predict_rank(Xq, Xc, T, exclude, rq, rc)
        return TargetRanks(rank, value, n_candidates)


_RANK_TARGETS_PER_CALL = 64  # (PAIRS_RANK_MAX_T of the device code)
TargetRanks = namedtuple("TargetRanks", ["rank", "value", "n_candidates"])
PairSummary = namedtuple("PairSummary", ["mean", "std"])
RankedSummary = namedtuple("RankedSummary", ["indices", "value", "mean", "std"])


class _PairUncertaintyMixin:
    """Ranking that counts what the model does not know yet, for the estimators that keep S posterior samples:
    the Gibbs regressor and classifier and MyFMOrderedProbit. The variational estimators keep one sample, the mean model, and so
    have no spread over samples; their spread is the analytic one of their Gaussian posterior, and they rank by it with
    predict_topk_bound (_VariationalMomentsMixin). With v_s(u, i) the per-sample value of the pair -- the score for a regressor, Phi(score) for a
    classifier, the expected class index for ordered probit, i.e. what predict_dist / predict_expected_dist summarise per row --

        mean = sum_s v_s / S,    std = the population standard deviation (ddof = 0) of the v_s,    value = mean + beta * std.

    Sides, relation-block arguments, the disjoint-columns rule, the exclusions and the memory rule are _PairScoringMixin's; the
    arguments are validated on the host before the device is touched. S = 1 and identical samples give std == 0.0 exactly."""

    def predict_pairs_dist(self, X_query, X_cand, X_rel_query=[], X_rel_cand=[]):
        """PairSummary(mean (U, I), std (U, I)) of every pair. U * I > 2^24 is refused (ValueError): use predict_topk_ucb."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        return PairSummary(*predictor.predict_pairs_dist(Xq, Xc, rq, rc))

    def predict_topk_ucb(self, X_query, X_cand, k: int, beta: float = 1.0, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Per query row the k candidates of largest value = mean + beta * std: RankedSummary(indices int64 (U, k), value, mean,
        std), each row ordered by (value descending, candidate index ascending). beta may be any finite float: positive explores,
        negative gives a conservative list (a lower bound), 0 ranks by the mean through this path. `exclude` as in predict_topk.

        value is what the selection compared; mean and std are recomputed for the selected pairs with the factors summed in
        another order, so value equals mean + beta * std within rounding, not bit for bit. Where fewer than k candidates remain
        the tail is index -1, value -inf, mean and std NaN. 1 <= k <= 256 and a finite real beta, else ValueError."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, beta, exclude = _ranked_args(Xq, Xc, k, exclude, beta)
        return RankedSummary(*predictor.predict_topk_ucb(Xq, Xc, k, beta, exclude, rq, rc))

    # ---- ranking under each kept sample: the S kept samples are S complete models, and each ranks the candidates
    # of a query by its own v_s(u, i) under predict_topk's order. Not row-sharded, k <= 256, no variational estimator.
    def predict_topk_samples(self, X_query, X_cand, k: int, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Every kept sample's own list: SampleRankings(indices int64 (S, U, k), value (S, U, k)), indices[s, u] the k candidates
        of largest v_s(u, .) ordered by (value descending, candidate index ascending), bit for bit what predict_topk gives for
        a model that keeps sample s alone. Tail: index -1, value -inf. `exclude` and 1 <= k <= 256 as in predict_topk."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, _, exclude = _ranked_args(Xq, Xc, k, exclude)
        return SampleRankings(*predictor.predict_topk_samples(Xq, Xc, k, exclude, rq, rc))

    def predict_topk_thompson(self, X_query, X_cand, k: int, random_seed: int = 0, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Thompson sampling: for every query one kept sample is drawn and that sample's list is recommended.
        ThompsonRanking(indices int64 (U, k), value (U, k), sample int64 (U,)) with
        sample = np.random.default_rng(random_seed).integers(0, S, size=U), drawn on the host and returned, so a call is
        reproducible and auditable: row u equals predict_topk_samples(...)[.][sample[u], u] bit for bit. A query is contracted
        against its one sample, 1 / S of predict_topk's arithmetic. random_seed: a non-negative int, else ValueError."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, _, exclude = _ranked_args(Xq, Xc, k, exclude)
        if isinstance(random_seed, (bool, np.bool_)) or not isinstance(random_seed, (int, np.integer)) or random_seed < 0:
            raise ValueError("random_seed must be a non-negative integer")
        n_samples = len(predictor.samples)
        if n_samples == 0:
            raise RuntimeError("Told to predict but no sample available.")
        sample = np.random.default_rng(int(random_seed)).integers(0, n_samples, size=Xq.shape[0])
        idx, value = predictor.predict_topk_thompson(Xq, Xc, k, sample.astype(np.int32), exclude, rq, rc)
        return ThompsonRanking(idx, value, sample.astype(np.int64))

    def predict_topk_prob(self, X_query, X_cand, k: int, n_top: Optional[int] = None, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """The top-k inclusion probability P(candidate i is among query u's k best): the share of the kept samples whose own
        list (predict_topk_samples) holds i. TopKProbability(indices int64 (U, n_top), probability (U, n_top)): per query the
        n_top (default k) candidates of largest probability ordered by (probability descending, candidate index ascending);
        where fewer candidates got a vote the tail is index -1, probability 0.0. The lists are counted on the device and never
        reach the host. n_top: an int in [1, 256]; kept samples * k may not exceed TOPK_PROB_MAX_VOTES; else ValueError."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, _, exclude = _ranked_args(Xq, Xc, k, exclude)
        if n_top is not None and (isinstance(n_top, (bool, np.bool_)) or not isinstance(n_top, (int, np.integer)) or not 1 <= n_top <= 256):
            raise ValueError("n_top must be an integer in [1, 256]")
        n_top = k if n_top is None else n_top  # (a k out of range is refused as predict_topk refuses it)
        n_samples = len(predictor.samples)
        if 1 <= k <= 256 and n_samples * k > TOPK_PROB_MAX_VOTES:  # (a k out of range is refused as predict_topk refuses it)
            raise ValueError("predict_topk_prob counts at most %d list entries per query (kept samples * k), this call has %d"
                             % (TOPK_PROB_MAX_VOTES, n_samples * k))
        return TopKProbability(*predictor.predict_topk_prob(Xq, Xc, k, int(n_top), exclude, rq, rc))


TOPK_PROB_MAX_VOTES = 32768  # (MFM_PAIRS_VOTE_MAX of the device code: a query's votes are sorted in the device's local memory)
SampleRankings = namedtuple("SampleRankings", ["indices", "value"])
ThompsonRanking = namedtuple("ThompsonRanking", ["indices", "value", "sample"])
TopKProbability = namedtuple("TopKProbability", ["indices", "probability"])


SIMILARITY_METRICS = ("cosine", "dot")


class _SimilarityMixin:
    """"Which items are like this item" (or user like this user) with a fitted model, for the estimators that keep S
    posterior samples. A side row a -- sparse in the model's feature space, with relation-block arguments as _PairScoringMixin takes
    them -- has the embedding P_s[a] = V_s^T a under kept sample s, and per sample

        cosine: c_s(a, b) = <P_s[a], P_s[b]> / (|P_s[a]| |P_s[b]|), 0 where a norm is 0 (an empty row, rank 0), not clamped;
        dot:    c_s(a, b) = <P_s[a], P_s[b]>;

        mean = sum_s c_s / S,    std = the population standard deviation of the c_s,    value = mean + beta * std.

    The kept samples' factors differ by signs and rotations, so the cosine of the averaged V means nothing; c_s is invariant under
    each sample's own rotation, which is also why a combine_chains result pools chains whose factors are rotated against each other.
    The task plays no part: w0, w and the cutpoints are not read. The two sides may store the same columns (items against items).
    Not covered: the variational estimators, row-sharded operation, other metrics. The arguments are validated on the host before the
    device is touched."""

    @staticmethod
    def _similarity_metric(metric):
        if not isinstance(metric, str) or metric not in SIMILARITY_METRICS:
            raise ValueError('metric must be "cosine" or "dot"')
        return metric

    def predict_similarity(self, X_a, X_b=None, metric="cosine", X_rel_a=[], X_rel_b=[]):
        """PairSummary(mean (U, I), std (U, I)) of the similarity of every row of X_a with every row of X_b (None: X_a itself, with
        X_rel_a). U * I > 2^24 is refused (ValueError): use predict_similar."""
        metric = self._similarity_metric(metric)
        if X_b is None:
            X_b, X_rel_b = X_a, X_rel_a
        predictor, Xa, Xb, ra, rb = self._pair_sides(X_a, X_b, X_rel_a, X_rel_b)
        return PairSummary(*predictor.predict_similarity(Xa, Xb, metric, ra, rb))

    def predict_similar(self, X_query, X_cand=None, k: int = 10, metric="cosine", beta: float = 0.0, exclude=None, exclude_self=None,
                        X_rel_query=[], X_rel_cand=[]):
        """Per query row the k candidates of largest value = mean + beta * std of the similarity: RankedSummary(indices int64 (U, k),
        value, mean, std), each row ordered by (value descending, candidate index ascending); tail index -1, value -inf, mean and
        std NaN. X_cand None: the candidates are the query rows themselves (with X_rel_query), and exclude_self, which then defaults
        to True, leaves every row out of its own list (the diagonal joins the exclusion pattern). exclude_self=True with an X_cand
        is a ValueError. `exclude`, k and beta as in predict_topk_ucb; mean and std are recomputed for the selected pairs with the
        factors summed in another order, so value equals mean + beta * std within rounding."""
        metric = self._similarity_metric(metric)
        same = X_cand is None
        if same:
            X_cand, X_rel_cand = X_query, X_rel_query
        elif exclude_self:
            raise ValueError("exclude_self needs the candidates to be the query rows (X_cand=None)")
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, beta, exclude = _ranked_args(Xq, Xc, k, exclude, beta)
        if same and (exclude_self is None or exclude_self):
            diag = sps.identity(Xq.shape[0], dtype=np.float64, format="csr")
            if exclude is not None:  # (the stored positions count, whatever their values)
                diag = sps.csr_matrix(sps.csr_matrix((np.ones(exclude.nnz), exclude.indices, exclude.indptr), shape=exclude.shape) + diag)
            exclude = diag
        return RankedSummary(*predictor.predict_similar(Xq, Xc, k, metric, beta, exclude, rq, rc))


def _fold_in_checked(est, name, X, y, entity, group, n_entities):
    """The host-side checks that fold_in and fold_in_gibbs share, in one order and with one set of messages (`name`: the calling
    method). Returns (predictor, D, K, X csr, y float64 (n,), entity int64 (n,), U, the hyper-parameters of the kept samples, group)."""
    predictor = est._fetch_predictor()
    D, K = int(predictor.feature_size), int(est.rank)
    if X is None or not sps.issparse(X):
        raise ValueError("X must be a scipy sparse matrix of shape (n, %d)" % D)
    X = _as_csr(X, 0)
    n = X.shape[0]
    if X.shape[1] != D:
        raise ValueError("X has %d columns but the fitted feature size is %d (the rows hold the context of the new "
                         "observations, not the new entity's column)" % (X.shape[1], D))
    y = np.asarray(y, dtype=REAL).reshape(-1)
    if y.shape[0] != n:
        raise ValueError("X has %d rows but y has %d entries" % (n, y.shape[0]))
    entity = np.asarray(entity)
    if entity.ndim != 1 or entity.shape[0] != n:
        raise ValueError("X has %d rows but entity has shape %s" % (n, entity.shape))
    if n and not np.issubdtype(entity.dtype, np.integer):
        raise ValueError("entity must hold integers")
    entity = entity.astype(np.int64)
    if n_entities is None:
        if n == 0:
            raise ValueError("an empty entity array needs n_entities")
        U = int(entity.max()) + 1
    else:
        if isinstance(n_entities, bool) or int(n_entities) != n_entities or n_entities < 0:
            raise ValueError("n_entities must be a non-negative integer")
        U = int(n_entities)
    if n and entity.min() < 0:
        raise ValueError("entity holds a negative index")
    if n and entity.max() >= U:
        raise ValueError("entity holds index %d but n_entities is %d" % (int(entity.max()), U))
    if not np.all(np.isfinite(y)):
        raise ValueError("y holds a value that is not finite")
    G = est.n_groups_ if est.n_groups_ is not None else 0
    if isinstance(group, bool) or not isinstance(group, (int, np.integer)) or not 0 <= group < G:
        raise ValueError("group must be an integer in [0, %d)" % G)
    if K > FOLD_IN_MAX_RANK:
        raise ValueError("%s serves ranks up to %d, this model has rank %d" % (name, FOLD_IN_MAX_RANK, K))
    n_samples = len(predictor.samples)
    hypers = None if est.history_ is None else est.history_.hypers
    if hypers is None or len(hypers) < n_samples:
        raise RuntimeError("%s needs history_ with the hyper-parameters of every kept sample" % name)
    return predictor, D, K, X, y, entity, U, hypers[len(hypers) - n_samples:], int(group)


def _fold_in_prior(kept, g, K):
    """(mu, lam), each (S, K + 1): per kept sample the prior mean and precision of (w, V_1 .. V_K) in group g"""
    mu = np.empty((len(kept), K + 1), dtype=REAL)
    lam = np.empty((len(kept), K + 1), dtype=REAL)
    for s, h in enumerate(kept):
        mu[s, 0], lam[s, 0] = np.asarray(h.mu_w)[g], np.asarray(h.lambda_w)[g]
        mu[s, 1:], lam[s, 1:] = np.asarray(h.mu_V)[g, :K], np.asarray(h.lambda_V)[g, :K]
    return mu, lam


def _fold_in_grouping(entity, U):
    """the observations grouped by entity (stable: an entity's rows keep their order): (order, offsets (U + 1,))"""
    order = np.argsort(entity, kind="stable")
    offsets = np.zeros(U + 1, dtype=np.int64)
    np.cumsum(np.bincount(entity, minlength=U), out=offsets[1:])
    return order, offsets


def _folded_in(est, predictor, D, U, group):
    """a new estimator of est's class around the extended predictor: constructor arguments, history_, n_groups_ and the chain count
    of a combined model carried over, grouping_ (where est has one) with `group` for the U new columns"""
    out = _unfitted_copy(est)
    out.predictor_ = predictor
    out.history_ = est.history_
    out.n_groups_ = est.n_groups_
    if hasattr(est, "grouping_"):
        g = est.grouping_
        out.grouping_ = None if g is None else np.concatenate([np.asarray(g, dtype=np.int32), np.full(U, group, dtype=np.int32)])
    out.fold_in_columns_ = (D, D + U)
    if hasattr(est, "n_chains_"):
        out.n_chains_ = est.n_chains_
    return out


def _unfitted_copy(est, random_seed=None):
    """a new, unfitted Gibbs estimator of est's class with its constructor arguments (`random_seed`: another seed)"""
    return type(est)(est.rank, init_stdev=est.init_stdev, random_seed=est.random_seed if random_seed is None else random_seed,
                     alpha_0=est.alpha_0, beta_0=est.beta_0, gamma_0=est.gamma_0, mu_0=est.mu_0, reg_0=est.reg_0, fit_w0=est.fit_w0,
                     fit_linear=est.fit_linear, exact_latent_draws=est.exact_latent_draws)


FOLD_IN_GIBBS_MAX_SWEEPS = 65535  # n_burn + n_inner: the sweep number is part of the random streams' draw word


class _FoldInGibbsMixin:
    """fold_in for the probit estimators: the new features' parameters have no closed-form posterior there, so each (entity, sample)
    runs a short Albert-Chib chain on the device."""

    def _fold_in_gibbs(self, X, y, entity, group, n_entities, draw, random_seed, n_burn, n_inner, cutpoint_index):
        for name, v, lo in (("n_burn", n_burn, 0), ("n_inner", n_inner, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
                raise ValueError("%s must be an integer of at least %d" % (name, lo))
        if n_burn + n_inner > FOLD_IN_GIBBS_MAX_SWEEPS:
            raise ValueError("n_burn + n_inner must not exceed %d" % FOLD_IN_GIBBS_MAX_SWEEPS)
        predictor, D, K, X, y, entity, U, kept, g = _fold_in_checked(self, "fold_in_gibbs", X, y, entity, group, n_entities)
        mu, lam = _fold_in_prior(kept, g, K)
        o = 0 if self.fit_linear else 1
        if not (np.all(np.isfinite(lam[:, o:])) and np.all(lam[:, o:] > 0.0)):
            raise ValueError("a kept sample has a prior precision that is not positive and finite")
        if not np.all(np.isfinite(mu[:, o:])):
            raise ValueError("a kept sample has a prior mean that is not finite")
        if self._task_type == TaskType.ORDERED:
            if isinstance(cutpoint_index, bool) or not isinstance(cutpoint_index, (int, np.integer)):
                raise ValueError("cutpoint_index must be an integer")
            samples = predictor.samples
            sizes = set(len(fm.cutpoints[cutpoint_index]) if 0 <= cutpoint_index < len(fm.cutpoints) else 0 for fm in samples)
            if 0 in sizes:
                raise ValueError("cutpoint_index %d out of range: a kept sample has no such cutpoint group" % cutpoint_index)
            if len(sizes) > 1:
                raise ValueError("the kept samples hold different numbers of cutpoints in group %d" % cutpoint_index)
            cut = np.asarray([fm.cutpoints[cutpoint_index] for fm in samples], dtype=REAL)
            if not np.all(np.isfinite(cut)):
                raise ValueError("a kept sample has a cutpoint that is not finite")
            if np.any(np.diff(cut, axis=1) < 0.0):
                raise ValueError("the cutpoints of a kept sample are not non-decreasing")
            n_class = cut.shape[1] + 1
            if np.any(y != np.floor(y)) or np.any(y < 0) or np.any(y >= n_class):
                raise ValueError("y must hold integer class labels in [0, %d)" % n_class)
        order, offsets = _fold_in_grouping(entity, U)
        w_new, V_new = predictor.fold_in_gibbs_solve(X[order], np.ascontiguousarray(y[order]), offsets, bool(self.fit_linear), mu, lam,
                                                     int(cutpoint_index), int(n_burn), int(n_inner), bool(draw),
                                                     int(random_seed) & 0xFFFFFFFFFFFFFFFF)
        return _folded_in(self, predictor.extended(w_new, V_new), D, U, g)


class MyFMGibbsBase(_FMEstimatorBase):
    """Common part of the Gibbs estimators (base.py:70-323 + gibbs.py:32-142)."""

    @property
    def w0_samples(self):
        if self.predictor_ is None:
            return None
        return np.asarray([fm.w0 for fm in self.predictor_.samples], dtype=REAL)

    @property
    def w_samples(self):
        if self.predictor_ is None:
            return None
        return np.asarray([fm.w for fm in self.predictor_.samples], dtype=REAL)

    @property
    def V_samples(self):
        if self.predictor_ is None:
            return None
        return np.asarray([fm.V for fm in self.predictor_.samples], dtype=REAL)

    def get_hyper_trace(self):
        """alpha, mu_w[g], lambda_w[g], mu_V[g,r], lambda_V[g,r] per iteration (gibbs.py:109-142)."""
        import pandas as pd

        if self.n_groups_ is None or self.history_ is None:
            raise RuntimeError("Sampler not run yet.")
        G, K = self.n_groups_, self.rank
        columns = (
            ["alpha"]
            + ["mu_w[{}]".format(g) for g in range(G)]
            + ["lambda_w[{}]".format(g) for g in range(G)]
            + ["mu_V[{},{}]".format(g, r) for g in range(G) for r in range(K)]
            + ["lambda_V[{},{}]".format(g, r) for g in range(G) for r in range(K)]
        )
        rows = []
        for hyper in self.history_.hypers:
            parts = [np.asarray([hyper.alpha])]
            for hp in (hyper.mu_w, hyper.lambda_w, hyper.mu_V, hyper.lambda_V):
                parts.append(np.asarray(hp, dtype=REAL).ravel())  # C-order ravel of (G, K): g outer, r inner
            rows.append(np.concatenate(parts))
        df = pd.DataFrame(np.vstack(rows))
        df.columns = columns
        return df


class MyFMGibbsRegressor(_PairScoringMixin, _PairUncertaintyMixin, _SimilarityMixin, _PredictiveDistMixin, _LooMixin, _DiagnosticsMixin, _CrpsMixin, _ContributionsMixin, MyFMGibbsBase):
    """Bayesian FM regression by Gibbs sampling (gibbs.py:145-240)."""

    _task_type = TaskType.REGRESSION

    def _prepare_prediction_for_test(self, fm, X, X_rel):
        return fm.predict_score(X, list(X_rel))

    def _status_report(self, fm, hyper) -> str:
        return "alpha = {:.2f} w0 = {:.2f} ".format(hyper.alpha, fm.w0)

    def _measure_score(self, prediction, y):
        y = np.asarray(y)
        out = OrderedDict()
        out["rmse"] = ((y - prediction) ** 2).mean() ** 0.5
        out["mae"] = np.abs(y - prediction).mean()
        return out

    def fit(self, X, y, X_rel=[], X_test=None, y_test=None, X_rel_test=[], n_iter=100, n_kept_samples=None, grouping=None,
            group_shapes=None, callback=None, config_builder=None):
        self._fit(X, y, X_rel=X_rel, X_test=X_test, y_test=y_test, X_rel_test=X_rel_test, n_iter=n_iter,
                  n_kept_samples=n_kept_samples, grouping=grouping, group_shapes=group_shapes, callback=callback,
                  config_builder=config_builder)
        return self

    def predict(self, X, X_rel=[], n_workers: Optional[int] = None):
        """Posterior predictive mean (gibbs.py:219-240)."""
        return self._predict_core(X, X_rel, n_workers=n_workers)

    def fold_in(self, X, y, entity, group, n_entities=None, draw=False, random_seed=0):
        """The fitted model extended by U new one-hot features -- users or items that were not in the training table and have
        now been observed a few times -- without refitting the chain. Returns a new MyFMGibbsRegressor of feature
        size D + U; this one is left untouched.

        X (n, D) scipy sparse, D the fitted feature size: the CONTEXT of each new observation in the model's full feature space
        (for a new user: the item's one-hot and whatever else the row carries), without the new entity's own column; a model
        fitted with relation blocks takes the expanded rows. y (n,): the targets. entity (n,): integers in [0, U) naming the new
        entity of each observation, in any order; an entity may have no observation. U = n_entities, or entity.max() + 1 when
        that is None. group: the prior group in [0, n_groups_) the new features belong to (the users' group for new users).

        A new feature with value 1 enters the score linearly, so under kept sample s its parameters theta = (w_u, V_u1 .. V_uK)
        have an exact Gaussian posterior given that sample's noise precision alpha_s and its group's mu_w, lambda_w, mu_V,
        lambda_V (the last S entries of history_.hypers, as predict_dist(noise=True) reads them):
            Lambda = diag(lambda) + alpha_s sum_i z_i z_i^T,   b = diag(lambda) mu + alpha_s sum_i z_i r_i,
            z_i = (1, q_s(x_i)),  q_sk(x) = sum_j V_s[j, k] x_j,  r_i = y_i - score_s(x_i),
        computed on the device per (entity, sample). draw=False stores the posterior mean Lambda^-1 b; draw=True stores a draw
        from the posterior, reproducible for random_seed. An entity without observations gets the prior mean (or a prior draw).
        A model fitted with fit_linear=False gets w_u = 0; rank 0 estimates w_u alone.

        The result's sample s is this model's sample s with w and V extended by the columns D .. D + U - 1 in entity order;
        cutpoints, history_, n_groups_ and the constructor arguments are carried over and fold_in_columns_ = (D, D + U). A query
        row for new entity u is the one-hot of column D + u (plus its context); predict, predict_dist, predict_pairs,
        predict_topk, w_samples, V_samples and pickling work on it as on any fitted model, and folding in twice (users, then
        items) composes. Its samples are host copies, the path of an unpickled model.

        Not covered: the variational estimators (MyFMGibbsClassifier and MyFMOrderedProbit have fold_in_gibbs, which runs a
        latent-variable inner chain); X_rel arguments; new features with a value other than 1; row-sharded operation (the model is replicated, so each
        rank can fold in its own entities). Ranks up to FOLD_IN_MAX_RANK. The arguments are checked on the host before the
        device is touched (ValueError)."""
        predictor, D, K, X, y, entity, U, kept, g = _fold_in_checked(self, "fold_in", X, y, entity, group, n_entities)
        alpha = np.asarray([h.alpha for h in kept], dtype=REAL)
        mu, lam = _fold_in_prior(kept, g, K)
        order, offsets = _fold_in_grouping(entity, U)
        w_new, V_new = predictor.fold_in_solve(X[order], np.ascontiguousarray(y[order]), offsets, bool(self.fit_linear), alpha, mu,
                                               lam, bool(draw), int(random_seed) & 0xFFFFFFFFFFFFFFFF)
        return _folded_in(self, predictor.extended(w_new, V_new), D, U, g)


class MyFMGibbsClassifier(_PairScoringMixin, _PairUncertaintyMixin, _SimilarityMixin, _PredictiveDistMixin, _LooMixin, _DiagnosticsMixin, _CrpsMixin, _ContributionsMixin, _FoldInGibbsMixin, MyFMGibbsBase):
    """Bayesian FM probit classification (gibbs.py:243-371)."""

    _task_type = TaskType.CLASSIFICATION

    def _process_y(self, y):
        return np.asarray(y).astype(REAL) * 2 - 1  # base.py:385-386

    def _prepare_prediction_for_test(self, fm, X, X_rel):
        return std_cdf(fm.predict_score(X, list(X_rel)))

    def _status_report(self, fm, hyper) -> str:
        return "w0 = {:.2f} ".format(fm.w0)

    def _measure_score(self, prediction, y):
        y = np.asarray(y)
        out = OrderedDict()
        lp = np.log(prediction + 1e-15)
        l1mp = np.log(1 - prediction + 1e-15)
        gt = y > 0
        out["ll"] = (-lp.dot(gt) - l1mp.dot(~gt)) / max(1, prediction.shape[0])
        out["accuracy"] = np.mean((prediction >= 0.5) == gt)
        return out

    def fit(self, X, y, X_rel=[], X_test=None, y_test=None, X_rel_test=[], n_iter=100, n_kept_samples=None, grouping=None,
            group_shapes=None, callback=None, config_builder=None):
        self._fit(X, y, X_rel=X_rel, X_test=X_test, y_test=y_test, X_rel_test=X_rel_test, n_iter=n_iter,
                  n_kept_samples=n_kept_samples, grouping=grouping, group_shapes=group_shapes, callback=callback,
                  config_builder=config_builder)
        return self

    def predict_proba(self, X, X_rel=[], n_workers: Optional[int] = None):
        return self._predict_core(X, X_rel, n_workers=n_workers)

    def predict(self, X, X_rel=[], n_workers: Optional[int] = None):
        return self.predict_proba(X, X_rel, n_workers=n_workers) > 0.5

    def fold_in_gibbs(self, X, y, entity, group, n_entities=None, draw=False, random_seed=0, n_burn=10, n_inner=40):
        """The fitted classifier extended by U new one-hot features (users or items that were not in the training table) from a few
        observations each, without refitting. Returns a new MyFMGibbsClassifier of feature size D + U; this one is
        left untouched. X, entity, group and n_entities are MyFMGibbsRegressor.fold_in's, checked the same way; y (n,) holds 0 / 1
        or bool labels as fit takes them.

        Under kept sample s the new feature's theta = (w_u, V_u1 .. V_uK) enters the score linearly, but a probit likelihood leaves
        no closed-form posterior: each (entity, sample) runs a chain of n_burn + n_inner Albert-Chib sweeps on the device (draw the
        latent of every observation truncated by its label, then theta from its Gaussian conditional), started at the prior mean.
        draw=False stores the Rao-Blackwellised posterior mean over the last n_inner sweeps; draw=True stores the chain's last
        state, a posterior draw. Both are reproducible for random_seed. n_burn + n_inner <= 65535. An entity without observations
        gets the prior mean (or a prior draw); fit_linear=False gives w_u = 0.

        The result is as fold_in's: history_, n_groups_ and the constructor arguments carried over, fold_in_columns_ = (D, D + U);
        predict_proba, predict_dist, predict_pairs, predict_topk and pickling work on it, and folding in twice composes. Not
        covered: X_rel arguments, features with a value other than 1, row-sharded operation. Ranks up to FOLD_IN_MAX_RANK. The
        arguments are checked on the host before the device is touched (ValueError)."""
        if self.predictor_ is not None and y is not None:
            y = self._process_y(y)
        return self._fold_in_gibbs(X, y, entity, group, n_entities, draw, random_seed, n_burn, n_inner, 0)


def _device_row_order(X):
    """stable order of the rows by their first stored column, or None when they already are (or it does not apply)"""
    import os

    if os.environ.get("MYFM_AMD_KEEP_ROW_ORDER") or X.shape[0] < 2 or X.shape[1] == 0:
        return None
    lens = np.diff(X.indptr)
    if lens.min() < 1:
        return None
    if not X.has_sorted_indices:
        X.sort_indices()
    first = X.indices[X.indptr[:-1]]
    if np.all(first[1:] >= first[:-1]):
        return None
    return _myfm.row_order_by_first_column(X.indptr, X.indices, X.shape[1])  # (stable counting sort)


class MyFMOrderedProbit(_PairScoringMixin, _PairUncertaintyMixin, _SimilarityMixin, _LooMixin, _DiagnosticsMixin, _CrpsMixin, _ContributionsMixin, _FoldInGibbsMixin, MyFMGibbsBase):
    """Bayesian FM ordinal regression (gibbs.py:374-543). predict_pairs / predict_topk rank by the posterior mean of the expected
    class index (see _PairScoringMixin). predict_proba_dist / predict_expected_dist give the posterior mean, standard deviation and
    quantiles of every class probability and of the expected class index over the kept samples."""

    _task_type = TaskType.ORDERED

    def _process_y(self, y):
        y = np.asarray(y)
        assert y.min() >= 0
        return y.astype(REAL)

    def fit(self, X, y, X_rel=[], X_test=None, y_test=None, X_rel_test=[], n_iter=100, n_kept_samples=None, grouping=None,
            group_shapes=None, callback=None, callback_default_freq=5):
        builder = ConfigBuilder()
        y = np.asarray(y)
        n_class = int(y.max()) + 1
        groups = [(n_class, np.arange(y.shape[0], dtype=np.int64))]
        self.n_cutpoint_groups = len(groups)
        builder.set_cutpoint_groups(groups)
        self._fit(X, y, X_rel=X_rel, X_test=X_test, y_test=y_test, X_rel_test=X_rel_test, n_iter=n_iter,
                  n_kept_samples=n_kept_samples, grouping=grouping, group_shapes=group_shapes, callback=callback,
                  config_builder=builder, callback_default_freq=callback_default_freq)
        return self

    def _prepare_prediction_for_test(self, fm, X, X_rel):
        return fm.oprobit_predict_proba(sps.csr_matrix(X, dtype=REAL), list(X_rel), 0)

    def _measure_score(self, prediction, y):
        y = np.asarray(y)
        out = OrderedDict()
        out["accuracy"] = (np.argmax(prediction, axis=1) == y).mean()
        out["log_loss"] = -np.log(prediction[np.arange(prediction.shape[0]), y.astype(np.int64)] + 1e-15).mean()
        return out

    def _status_report(self, fm, hyper) -> str:
        msg = "w0 = {:.2f}, ".format(fm.w0)
        cps = fm.cutpoints
        if len(cps) == 1:
            msg += "cutpoint = {} ".format(["{:.3f}".format(c) for c in list(cps[0])])
        return msg

    def predict_proba(self, X, X_rel=[], n_workers: Optional[int] = None):
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        return predictor.predict_parallel_oprobit(X, list(X_rel), n_workers or 1, 0)

    def predict(self, X, X_rel=[]):
        return self.predict_proba(X, X_rel=X_rel).argmax(axis=1)

    def fold_in_gibbs(self, X, y, entity, group, n_entities=None, draw=False, random_seed=0, n_burn=10, n_inner=40, cutpoint_index=0):
        """MyFMGibbsClassifier.fold_in_gibbs for ordered probit: y (n,) holds integer class labels in [0, n_class), n_class the
        number of cutpoints of group `cutpoint_index` of the kept samples plus one (checked as predict_proba_dist checks it). A
        latent is drawn between its class's cutpoints of that sample. Returns a new MyFMOrderedProbit of feature size D + U with
        the cutpoints carried over; predict_proba, predict_proba_dist, predict_expected_dist, predict_topk and pickling work on it."""
        out = self._fold_in_gibbs(X, y, entity, group, n_entities, draw, random_seed, n_burn, n_inner, cutpoint_index)
        if hasattr(self, "n_cutpoint_groups"):
            out.n_cutpoint_groups = self.n_cutpoint_groups
        return out

    def _predict_dist_oprobit(self, X, X_rel, quantiles, cutpoint_index, expected):
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        probs = _checked_quantiles(quantiles)
        samples = predictor.samples
        _check_sample_limit(probs, len(samples))
        if isinstance(cutpoint_index, bool) or not isinstance(cutpoint_index, (int, np.integer)):
            raise ValueError("cutpoint_index must be an integer")
        sizes = set(len(fm.cutpoints[cutpoint_index]) if 0 <= cutpoint_index < len(fm.cutpoints) else 0 for fm in samples)
        if 0 in sizes:
            raise ValueError("cutpoint_index %d out of range: a kept sample has no such cutpoint group" % cutpoint_index)
        if len(sizes) > 1:
            raise ValueError("the kept samples hold different numbers of cutpoints in group %d" % cutpoint_index)
        return PredictiveSummary(*predictor.predict_dist_oprobit(X, list(X_rel), probs, int(cutpoint_index), expected))

    def predict_proba_dist(self, X, X_rel=[], quantiles=(0.05, 0.5, 0.95), cutpoint_index=0):
        """PredictiveSummary(mean, std, quantiles) of every class probability over the S kept samples, computed on the device:
        the per-sample value is p_c(score_s; cutpoints_s), the probability of class c under sample s's score and sample s's
        own cutpoints, C = n_cut + 1 classes.

        mean (N, C): what predict_proba returns, bit for bit -- and, y being discrete, the predictive distribution of y itself
        (there is no `noise` argument). std (N, C): population standard deviation (ddof = 0). quantiles (Q, N, C):
        np.quantile(p, quantiles, axis=0) under the default "linear" rule, from exactly sorted values; `quantiles` may be empty
        (at most 32 entries in [0, 1]; S <= 4096 unless it is empty). The number of classes has no limit.

        The arguments are checked on the host before the device is touched."""
        return self._predict_dist_oprobit(X, X_rel, quantiles, cutpoint_index, False)

    def predict_expected_dist(self, X, X_rel=[], quantiles=(0.05, 0.5, 0.95), cutpoint_index=0):
        """As predict_proba_dist, of the expected class index sum_c c p_c (added in ascending class order), the value that
        predict_topk ranks by: mean (N,), std (N,), quantiles (Q, N)."""
        return self._predict_dist_oprobit(X, X_rel, quantiles, cutpoint_index, True)

    def predict_log_density(self, X, y, X_rel=[], pointwise=False, cutpoint_index=0):
        """_LogDensityMixin.predict_log_density with the cutpoint group to use: y (N,) holds integer class labels in [0, n_class),
        n_class the number of cutpoints of group `cutpoint_index` of the kept samples plus one."""
        return self._predict_log_density(X, y, X_rel, pointwise, cutpoint_index)

    def predict_loo(self, X, y, X_rel=[], log_weights=False, r_eff=1.0, cutpoint_index=0):
        """_LooMixin.predict_loo with the cutpoint group to use, as predict_log_density takes it."""
        return self._predict_loo(X, y, X_rel, log_weights, r_eff, cutpoint_index)

    def predict_loo_dist(self, X, y, X_rel=[], quantiles=(0.05, 0.5, 0.95), r_eff=1.0, cutpoint_index=0):
        """_LooMixin.predict_loo_dist of the expected class index sum_c c p_c under the cutpoints of group `cutpoint_index`, the
        value predict_expected_dist summarises."""
        return self._predict_loo_dist(X, y, X_rel, quantiles, r_eff, cutpoint_index)

    def predict_loo_crps(self, X, y, X_rel=[], r_eff=1.0, cutpoint_index=0):
        """_LooMixin.predict_loo_crps with the cutpoint group to use: the leave-one-out ranked probability score."""
        return self._predict_loo_crps(X, y, X_rel, r_eff, cutpoint_index)

    def predict_crps(self, X, y, X_rel=[], cutpoint_index=0):
        """_CrpsMixin.predict_crps with the cutpoint group to use, as predict_log_density takes it: the ranked probability score."""
        return self._predict_crps(X, y, X_rel, cutpoint_index)

    def predict_diagnostics(self, X, X_rel=[], cutpoint_index=0):
        """_DiagnosticsMixin.predict_diagnostics of the expected class index sum_c c p_c under the cutpoints of group
        `cutpoint_index`, the value predict_expected_dist summarises and predict_topk ranks by."""
        return self._predict_diagnostics(X, X_rel, cutpoint_index)

    def likelihood_diagnostics(self, X, y, X_rel=[], cutpoint_index=0):
        """_DiagnosticsMixin.likelihood_diagnostics with the cutpoint group to use, as predict_log_density takes it."""
        return self._likelihood_diagnostics(X, y, X_rel, cutpoint_index)

    @property
    def cutpoint_samples(self):
        if self.predictor_ is None:
            return None
        return np.asarray([fm.cutpoints[0] for fm in self.predictor_.samples], dtype=REAL)


ScoreMoments = namedtuple("ScoreMoments", ["mean", "std"])


class _VariationalMomentsMixin:
    """What the variational posterior knows about a score. The variational estimators keep one model, but that model
    is a full mean-field Gaussian posterior -- w0 ~ N(w0_mean, w0_var), w ~ N(w_mean, w_var), V ~ N(V_mean, V_var), independent --
    under which the FM score of a row has a closed-form mean (the mean model's score, what predict returns) and variance

        Var[score] = w0_var + sum x^2 w_var + sum_k [ M^2 A - 2 M B + C + (A^2 - E) / 2 ]_k,
        M = sum x m,  A = sum x^2 s,  B = sum x^3 s m,  C = sum x^4 s m^2,  E = sum x^4 s^2     (m = V_mean, s = V_var, per factor).

    The score is not Gaussian; these are its two exact moments, computed on the device for design rows (relation blocks are never
    expanded) and for every (query, candidate) pair, with the top k by mean + beta * std fused into the pair kernel. Sides,
    relation-block arguments, the disjoint-columns rule, the exclusions and the memory rule are _PairScoringMixin's; the arguments
    are validated on the host before the device is touched. Not row-sharded: the model is replicated, so each rank calls on its own
    rows. Everything here reads the six posterior arrays alone, so it works on an unpickled estimator."""

    def _noise_variance(self, noise):
        if not noise:
            return 0.0
        if self._task_type != TaskType.REGRESSION:
            raise ValueError("noise=True describes a regression target: it is not available on a classifier")
        hyper = None if self.history_ is None else self.history_.hypers
        if hyper is None or not np.isfinite(hyper.alpha) or not hyper.alpha > 0.0:
            raise RuntimeError("noise=True needs history_ with the fitted noise precision alpha")
        return 1.0 / float(hyper.alpha)

    def predict_moments(self, X, X_rel=[], noise=False):
        """ScoreMoments(mean (N,), std (N,)) of the score of every row. mean is predict() of the regressor (the mean model's score
        for the classifier) bit for bit on a design without relation blocks; std = sqrt(max(Var[score], 0)). noise=True (regressor
        only, ValueError on the classifier) describes y itself: 1 / alpha, alpha the fitted noise precision (history_.hypers.alpha),
        is added to the variance."""
        predictor = self._fetch_predictor()
        extra_var = self._noise_variance(noise)
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        return ScoreMoments(*predictor.predict_moments(X, list(X_rel), extra_var, False))

    def predict_pairs_moments(self, X_query, X_cand, X_rel_query=[], X_rel_cand=[]):
        """PairSummary(mean (U, I), std (U, I)) of the SCORE of every pair, for both estimators; mean is the regressor's
        predict_pairs bit for bit. U * I > 2^24 is refused (ValueError): use predict_topk_bound."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        return PairSummary(*predictor.predict_pairs_moments(Xq, Xc, rq, rc))

    def predict_topk_bound(self, X_query, X_cand, k: int, beta: float = 1.0, exclude=None, X_rel_query=[], X_rel_cand=[]):
        """Per query row the k candidates of largest value = mean + beta * std of the score: RankedSummary(indices int64 (U, k),
        value, mean, std), each row ordered by (value descending, candidate index ascending). beta may be any finite float:
        positive ranks by an optimistic bound, negative by a conservative one, 0 by the mean. For the classifier this ranks by a
        quantile of the probability: Phi is monotone, so the order of mean + beta * std of the score is the order of Phi of it.
        `exclude` as in predict_topk.

        value is what the selection compared; mean and std are recomputed for the selected pairs with the factors summed in another
        order, so value equals mean + beta * std within rounding. Where fewer than k candidates remain the tail is index -1, value
        -inf, mean and std NaN. 1 <= k <= 256 and a finite real beta, else ValueError."""
        predictor, Xq, Xc, rq, rc = self._pair_sides(X_query, X_cand, X_rel_query, X_rel_cand)
        k, beta, exclude = _ranked_args(Xq, Xc, k, exclude, beta)
        return RankedSummary(*predictor.predict_topk_bound(Xq, Xc, k, beta, exclude, rq, rc))


class MyFMVariationalBase(_FMEstimatorBase):
    """Common part of the variational estimators (src/myfm/variational.py:40-167): the same arguments as the Gibbs
    estimators (exact_latent_draws does not apply), and the posterior means and variances of the final model."""

    _variational = True

    def __init__(self, rank: int, init_stdev: float = 0.1, random_seed: int = 42, alpha_0: float = 1.0, beta_0: float = 1.0,
                 gamma_0: float = 1.0, mu_0: float = 0.0, reg_0: float = 1.0, fit_w0: bool = True, fit_linear: bool = True):
        super().__init__(rank, init_stdev=init_stdev, random_seed=random_seed, alpha_0=alpha_0, beta_0=beta_0, gamma_0=gamma_0,
                         mu_0=mu_0, reg_0=reg_0, fit_w0=fit_w0, fit_linear=fit_linear)
        del self.exact_latent_draws  # (a Gibbs option)

    def _weight(self, name):
        if self.predictor_ is None:
            return None
        return getattr(self.predictor_.weights(), name)

    @property
    def w0_mean(self):
        return self._weight("w0")

    @property
    def w0_var(self):
        return self._weight("w0_var")

    @property
    def w_mean(self):
        return self._weight("w")

    @property
    def w_var(self):
        return self._weight("w_var")

    @property
    def V_mean(self):
        return self._weight("V")

    @property
    def V_var(self):
        return self._weight("V_var")

    def _fit_vb(self, X, y, X_rel, X_test, y_test, X_rel_test, n_iter, grouping, group_shapes, callback, config_builder):
        self._fit(X, y, X_rel=X_rel, X_test=X_test, y_test=y_test, X_rel_test=X_rel_test, n_iter=n_iter, grouping=grouping,
                  group_shapes=group_shapes, callback=callback, config_builder=config_builder)
        return self


class VariationalFMRegressor(_PairScoringMixin, _VariationalMomentsMixin, MyFMVariationalBase):
    """Bayesian FM regression by mean-field variational inference (variational.py:170-265)."""

    # the task hooks of the regression estimators (the two families are siblings, as in the reference)
    _task_type = TaskType.REGRESSION
    _prepare_prediction_for_test = MyFMGibbsRegressor._prepare_prediction_for_test
    _status_report = MyFMGibbsRegressor._status_report
    _measure_score = MyFMGibbsRegressor._measure_score

    def fit(self, X, y, X_rel=[], X_test=None, y_test=None, X_rel_test=[], n_iter=100, grouping=None, group_shapes=None,
            callback=None, config_builder=None):
        return self._fit_vb(X, y, X_rel, X_test, y_test, X_rel_test, n_iter, grouping, group_shapes, callback, config_builder)

    def predict(self, X, X_rel=[]):
        """The score of the mean model (variational.py:248-265)."""
        return self._predict_core(X, X_rel)


class VariationalFMClassifier(_PairScoringMixin, _VariationalMomentsMixin, MyFMVariationalBase):
    """Bayesian FM probit classification by mean-field variational inference (variational.py:268-383)."""

    _task_type = TaskType.CLASSIFICATION
    _process_y = MyFMGibbsClassifier._process_y
    _prepare_prediction_for_test = MyFMGibbsClassifier._prepare_prediction_for_test
    _status_report = MyFMGibbsClassifier._status_report
    _measure_score = MyFMGibbsClassifier._measure_score

    def fit(self, X, y, X_rel=[], X_test=None, y_test=None, X_rel_test=[], n_iter=100, grouping=None, group_shapes=None,
            callback=None, config_builder=None):
        return self._fit_vb(X, y, X_rel, X_test, y_test, X_rel_test, n_iter, grouping, group_shapes, callback, config_builder)

    def predict_proba(self, X, X_rel=[]):
        """Phi of the mean model's score (variational.py:366-383)."""
        return self._predict_core(X, X_rel)

    def predict_proba_marginal(self, X, X_rel=[]):
        """(N,) Phi(mean / sqrt(1 + Var[score])): the probit link integrated over the score's posterior, the score taken as Gaussian
        with its two exact moments (predict_moments). predict_proba stays the mean model's Phi(mean); this one is pulled towards
        1/2 where the posterior is wide."""
        predictor = self._fetch_predictor()
        n = check_data_consistency(X, X_rel)
        X = _as_csr(X, n)
        return predictor.predict_moments(X, list(X_rel), 0.0, True)[2]

    def predict(self, X, X_rel=[]):
        return self.predict_proba(X, X_rel) > 0.5


MyFMRegressor = MyFMGibbsRegressor
MyFMClassifier = MyFMGibbsClassifier


# ---- several chains ----------------------------------------------------------------------------------------------
COMBINE_MAX_CHAINS = int(_myfm.ESS_MAX_CHAINS)  # (of the device code: the 2 x 32 half-chains of a row are the lanes of one wavefront)


def _kept_tail(entries, n):
    """the last n entries (those of the kept samples) of a per-iteration list of a history; a shorter list whole"""
    entries = list(entries)
    return entries[len(entries) - n:] if len(entries) >= n else entries


def combine_chains(estimators):
    """One model of the kept samples of several fits of the same model from different seeds -- M chains -- as a new estimator of
    their class; the inputs are left untouched. It holds the samples of chain 0, then chain 1, ... (host copies, the path of an
    unpickled model), n_chains_ = M, the constructor arguments and n_groups_ of the first input, and a history_ whose hypers are
    exactly the hyper-parameters of the kept samples in that order (train_log_losses and n_mh_accept likewise). Every predictor
    works on the pooled samples: predict*, predict_dist, pairs, top-k, ranking, log density, LOO, CRPS, fold_in, pickling.
    predict_diagnostics, likelihood_diagnostics and predict_loo(r_eff="auto") compare the chains: R-hat and the effective sample
    sizes are those of the 2M half-chains, after Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021).

    ValueError: an empty list; more than 32 estimators; estimators of different classes; a variational estimator; one that is not
    fitted, is itself combined, or differs from the first in rank, feature size, n_groups_, fold_in_columns_, the number of kept
    samples or the number of cutpoints."""
    ests = list(estimators)
    if not ests:
        raise ValueError("combine_chains needs at least one fitted estimator")
    first = ests[0]
    if any(type(e) is not type(first) for e in ests):
        raise ValueError("combine_chains needs estimators of one class, got %s" % sorted(set(type(e).__name__ for e in ests)))
    if getattr(first, "_variational", False) or not isinstance(first, MyFMGibbsBase):
        raise ValueError("combine_chains combines Gibbs chains: %s keeps no samples to pool" % type(first).__name__)
    if len(ests) > COMBINE_MAX_CHAINS:
        raise ValueError("at most %d chains are combined, got %d" % (COMBINE_MAX_CHAINS, len(ests)))
    for c, e in enumerate(ests):
        if e.predictor_ is None or e.history_ is None:
            raise ValueError("combine_chains: estimator %d is not fitted" % c)
        if getattr(e, "n_chains_", 1) != 1:
            raise ValueError("combine_chains: estimator %d is itself a combination of chains" % c)
    n_kept = len(first.predictor_.samples)

    def cut_sizes(e):
        samples = e.predictor_.samples
        return tuple(len(g) for g in samples[0].cutpoints) if len(samples) else ()

    for c, e in enumerate(ests):
        for what, a, b in (("rank", first.rank, e.rank), ("feature size", first.predictor_.feature_size, e.predictor_.feature_size),
                           ("n_groups_", first.n_groups_, e.n_groups_),
                           ("fold_in_columns_", getattr(first, "fold_in_columns_", None), getattr(e, "fold_in_columns_", None)),
                           ("number of kept samples", n_kept, len(e.predictor_.samples)),
                           ("number of cutpoints", cut_sizes(first), cut_sizes(e))):
            if a != b:
                raise ValueError("combine_chains: estimator %d differs from the first in its %s (%s, the first has %s)" % (c, what, b, a))
        if len(e.history_.hypers) < n_kept:
            raise ValueError("combine_chains: estimator %d has no history_ entry for every kept sample" % c)
    out = _unfitted_copy(first)
    out.predictor_ = _myfm.Predictor.concatenated([e.predictor_ for e in ests])
    out.history_ = _myfm.LearningHistory(
        [h for e in ests for h in _kept_tail(e.history_.hypers, n_kept)],
        [v for e in ests for v in _kept_tail(e.history_.train_log_losses, n_kept)],
        [v for e in ests for v in _kept_tail(e.history_.n_mh_accept, n_kept)])
    out.n_groups_ = first.n_groups_
    out.n_chains_ = len(ests)
    for name in ("fold_in_columns_", "n_cutpoint_groups", "grouping_"):
        if hasattr(first, name):
            setattr(out, name, getattr(first, name))
    return out


def fit_chains(estimator, X, y, n_chains=4, seeds=None, **fit_kwargs):
    """Fit `n_chains` fresh copies of the Gibbs `estimator` on X, y one after another, each from its own seed, and return
    combine_chains of them; `estimator` itself is left untouched. seeds: a list of n_chains distinct integers, by default
    estimator.random_seed + c for chain c, so that chain 0 is draw for draw what estimator.fit(X, y, **fit_kwargs) gives.
    fit_kwargs are fit's (X_rel, n_iter, n_kept_samples, grouping, ...). Each fit's samples leave the device as soon as they
    are copied: at no time does more than one chain's store live there. 1 <= n_chains <= 32. Not row-sharded: RuntimeError while
    myfm_amd.distributed is active."""
    from . import distributed as _dist

    if getattr(estimator, "_variational", False) or not isinstance(estimator, MyFMGibbsBase):
        raise ValueError("fit_chains runs Gibbs chains: %s keeps no samples to pool" % type(estimator).__name__)
    if isinstance(n_chains, (bool, np.bool_)) or not isinstance(n_chains, (int, np.integer)) or not 1 <= n_chains <= COMBINE_MAX_CHAINS:
        raise ValueError("n_chains must be an integer in [1, %d]" % COMBINE_MAX_CHAINS)
    if seeds is None:
        seeds = [int(estimator.random_seed) + c for c in range(n_chains)]
    else:
        seeds = list(seeds)
        if any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in seeds):
            raise ValueError("seeds must hold integers")
        seeds = [int(v) for v in seeds]
        if len(seeds) != n_chains or len(set(seeds)) != n_chains:
            raise ValueError("seeds must hold n_chains = %d distinct integers" % n_chains)
    if _dist.active():
        raise RuntimeError("fit_chains is not row-sharded: leave myfm_amd.distributed before running several chains")
    chains = []
    for seed in seeds:
        chain = _unfitted_copy(estimator, seed).fit(X, y, **fit_kwargs)
        chain.predictor_ = _myfm.Predictor.concatenated([chain.predictor_])  # (host copies: the fit's device store is released)
        chains.append(chain)
    return combine_chains(chains)
