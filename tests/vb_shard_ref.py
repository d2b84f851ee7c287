"""NumPy restatement of the ROW-SHARDED variational iteration (csrc/mfm_vb.hip, the split path): the rows of the expanded design
are cut into contiguous shards, each with its own e, q, x2s, x3sv; the model and the hyper-parameters are replicated. Per level
of the column schedule every shard forms the partial sums of its rows -- (sum x^2, sum x (e - x w_old)) for update_w, (sq, lin,
sq_var, lin_var) for update_V as they stand BEFORE `lin += sq * v_old` --, the partial sums are added over the shards (the
all-reduce), and the update is finished from the total: everything that multiplies by v_old, alpha or lambda happens after the
sum. The four score sums are added over the shards as well, and w0_var * N (N = all rows) is added once, after that sum.

`collectives` counts the sums over shards the way the device counts its all-reduces: one per non-empty level and sweep, one per
score pass. The host steps (alpha, w0, lambda, mu, the ELBO's model terms) are those of tests/vb_ref.py."""
import numpy as np
import scipy.sparse as sps

from . import vb_ref


def column_levels(X):
    """level(j) = 1 + the highest level of the earlier columns that share a row with j (mfm_common.hpp column_levels)"""
    Xt = sps.csr_matrix(X).T.tocsr()
    rowlevel = np.full(X.shape[0], -1, dtype=np.int64)
    level = np.zeros(X.shape[1], dtype=np.int32)
    for j in range(X.shape[1]):
        rows = Xt.indices[Xt.indptr[j]:Xt.indptr[j + 1]]
        level[j] = (rowlevel[rows].max() if rows.size else -1) + 1
        rowlevel[rows] = level[j]
    return level


class _Shard:
    def __init__(self, X, y):
        self.X = sps.csr_matrix(X, dtype=np.float64)
        self.Xt = self.X.T.tocsr()
        self.y = np.asarray(y, dtype=np.float64)
        n = self.X.shape[0]
        self.e, self.q, self.x2s, self.x3sv = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)

    def col(self, j):
        a, b = self.Xt.indptr[j], self.Xt.indptr[j + 1]
        return self.Xt.indices[a:b], self.Xt.data[a:b]


class ShardedVBRef(vb_ref.VBRef):
    """VBRef over the expanded (flat) design with its rows cut at `cuts` (world + 1 ascending row indices, equal neighbours
    = an empty shard)"""

    def __init__(self, X, y, rank, group_index, task, cfg, w0, w, V, init_std, blocks=(), cuts=None):
        Xf = sps.hstack([sps.csr_matrix(X)] + [sps.csr_matrix(B)[np.asarray(mp)] for mp, B in blocks]).tocsr() if blocks else X
        super().__init__(Xf, y, rank, group_index, task, cfg, w0, w, V, init_std)
        cuts = [0, self.N] if cuts is None else list(cuts)
        assert cuts[0] == 0 and cuts[-1] == self.N and all(a <= b for a, b in zip(cuts, cuts[1:]))
        self.cuts = cuts
        self.shards = [_Shard(self.X[a:b], self.y[a:b]) for a, b in zip(cuts, cuts[1:])]
        level = column_levels(self.X)
        self.levels = [np.nonzero(level == l)[0] for l in range(int(level.max()) + 1 if level.size else 0)]
        self.collectives = 0
        self.sums = self._score(0)  # initialize_e: e -= y for both tasks

    def _allreduce(self, parts):
        self.collectives += 1
        total = parts[0].copy()
        for p in parts[1:]:
            total = total + p
        return total

    # ---- the score pass: (sum e, sum e^2, sum of the per-row variance terms, likelihood term) per shard, then over shards
    def _score(self, mode):
        parts = []
        for s in self.shards:
            score, var = vb_ref.update_e_and_var(s.X, self.w0, 0.0, self.w, self.w_var, self.V, self.V_var)  # (no w0_var N here)
            lik = 0.0
            if mode == 0:
                s.e = score - s.y
            else:
                m_l, _, lz_l = vb_ref.truncated_normal_left(score)
                m_r, _, lz_r = vb_ref.truncated_normal_right(score)
                pos = s.y > 0
                m, lz = np.where(pos, m_l, m_r), np.where(pos, lz_l, lz_r)
                s.e = score - m
                lik = np.sum(lz + (m - score) ** 2 / 2)
            parts.append(np.array([s.e.sum(), np.sum(s.e**2), var, lik]))
        out = self._allreduce(parts)
        out[2] += self.w0_var * self.N  # once, after the sum over shards
        return out

    @property
    def e_all(self):
        return np.concatenate([s.e for s in self.shards])

    def step_alpha(self):
        if self.task == "classification":
            self.alpha, self.alpha_rate = 1.0, 1.0
            return
        rate = (self.cfg.beta_0 + self.sums[1] + self.sums[2]) / 2
        self.alpha, self.alpha_rate = (self.cfg.alpha_0 + self.N) / 2 / rate, rate

    def step_w0(self):
        if not self.cfg.fit_w0:
            self.w0 = self.w0_var = 0.0
            return
        lin = self.alpha * (self.w0 * self.N - self.sums[0])
        quad = self.alpha * self.N + self.cfg.reg_0
        new = lin / quad
        for s in self.shards:
            s.e = s.e + (new - self.w0)
        self.w0, self.w0_var = new, 1 / quad

    def sweep_w(self):
        for cols in self.levels:
            parts = []
            for s in self.shards:  # k_vb_stats_w
                S = np.zeros((len(cols), 2))
                for c, j in enumerate(cols):
                    rows, x = s.col(j)
                    S[c] = np.sum(x * x), np.sum(x * (s.e[rows] - x * self.w[j]))
                parts.append(S)
            S = self._allreduce(parts)
            for c, j in enumerate(cols):  # k_vb_apply_w: the same on every shard
                g = self.gi[j]
                w_old = self.w[j]
                square = self.lambda_w[g] + self.alpha * S[c, 0]
                linear = -self.alpha * S[c, 1] + self.lambda_w[g] * self.mu_w[g]
                w_new = linear / square
                for s in self.shards:
                    rows, x = s.col(j)
                    s.e[rows] = (s.e[rows] - x * w_old) + x * w_new
                self.w[j], self.w_var[j] = w_new, 1 / square

    def sweep_factor(self, r):
        v, sv = self.V[:, r], self.V_var[:, r]
        for s in self.shards:  # k_vb_cache
            X2 = s.X.multiply(s.X).tocsr()
            s.q, s.x2s, s.x3sv = s.X @ v, X2 @ sv, X2.multiply(s.X).tocsr() @ (sv * v)
        for cols in self.levels:
            parts = []
            for s in self.shards:  # k_vb_stats_v
                S = np.zeros((len(cols), 4))
                for c, j in enumerate(cols):
                    rows, x = s.col(j)
                    h = x * (s.q[rows] - x * v[j])
                    a2 = s.x2s[rows] - x * x * sv[j]
                    a3 = s.x3sv[rows] - x * x * x * sv[j] * v[j]
                    S[c] = np.sum(h * h), np.sum(-s.e[rows] * h), np.sum(a2 * x * x), np.sum(h * a2 - x * a3)
                parts.append(S)
            S = self._allreduce(parts)
            for c, j in enumerate(cols):  # k_vb_apply_v
                g = self.gi[j]
                v_old, s_old = v[j], sv[j]
                sq, lin, sq_var, lin_var = S[c]
                lin = lin + sq * v_old  # after the sum over shards
                lin -= lin_var
                sq = (sq + sq_var) * self.alpha + self.lambda_V[g, r]
                lin = lin * self.alpha + self.lambda_V[g, r] * self.mu_V[g, r]
                v_new, s_new = lin / sq, 1 / sq
                for s in self.shards:
                    rows, x = s.col(j)
                    h = x * (s.q[rows] - x * v_old)
                    s.q[rows] += x * (v_new - v_old)
                    s.e[rows] += h * (v_new - v_old)
                    s.x2s[rows] += x * x * (s_new - s_old)
                    s.x3sv[rows] += x * x * x * (s_new * v_new - s_old * v_old)
                v[j], sv[j] = v_new, s_new

    def step_e(self):
        c = self.cfg
        self.sums = self._score(1 if self.task == "classification" else 0)
        elbo = self.sums[3] if self.task == "classification" else 0.0
        elbo += -self.alpha * (c.beta_0 + self.sums[1] + self.sums[2]) / 2
        elbo += self.alpha * self.alpha_rate * (1 - np.log(self.alpha_rate))
        with np.errstate(divide="ignore"):
            elbo += -c.gamma_0 * (self.w0 * self.w0 + self.w0_var) + 0.5 * np.log(self.w0_var)
        for g, f in enumerate(self.groups):  # features are replicated: no sum over shards
            elbo += 0.5 * np.log(self.mu_w_var[g]) + 0.5 * np.sum(np.log(self.w_var[f]))
            rate = c.beta_0 + np.sum((self.w[f] - self.mu_w[g]) ** 2 + self.mu_w_var[g] + self.w_var[f])
            elbo += self.lambda_w[g] * (-rate / 2 + self.lambda_w_rate[g])
            elbo -= self.lambda_w[g] * self.lambda_w_rate[g] * np.log(self.lambda_w_rate[g])
            elbo += -((self.mu_w[g] - c.mu_0) ** 2) / 2
            for r in range(self.K):
                elbo += 0.5 * np.log(self.mu_V_var[g, r]) + 0.5 * np.sum(np.log(self.V_var[f, r]))
                rate = c.beta_0 + np.sum((self.V[f, r] - self.mu_V[g, r]) ** 2 + self.mu_V_var[g, r] + self.V_var[f, r])
                elbo += self.lambda_V[g, r] * (-rate / 2 + self.lambda_V_rate[g, r])
                elbo -= self.lambda_V[g, r] * self.lambda_V_rate[g, r] * np.log(self.lambda_V_rate[g, r])
        self.elbos.append(elbo)
