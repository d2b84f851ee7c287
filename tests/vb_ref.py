"""NumPy restatement of the reference's VariationalFMTrainer (include/myfm/variational.hpp:147-918) over a main table without
relation blocks, written from its statements: initialize_hyper (:219-232), initialize_e (:234-241), and per iteration
update_alpha (:248-266), update_w0 (:348-361), update_lambda_w / update_mu_w (:269-318), update_w (:363-386),
update_lambda_V / update_mu_V, update_V (:450-554) and update_e with the ELBO (:715-918). The coordinate sweeps run feature
after feature, as the reference does; only the sums inside one feature's statistics are vectorised."""
import numpy as np
import scipy.sparse as sps
from scipy import special

SQRT2 = 1.4142135623730951
SQRT2PI = SQRT2 * 1.7724538509055159


def truncated_normal_left(mu):
    """(mean, var, lnZ) of N(mu, 1) truncated to z > 0 (util.hpp:80-107), elementwise"""
    mu = np.asarray(mu, dtype=np.float64)
    phi_Z = np.exp(-mu * mu / 2 - special.log_ndtr(mu)) / np.sqrt(2 * np.pi)
    return mu + phi_Z, 1 - mu * phi_Z - phi_Z * phi_Z, np.log(2.0) + special.log_ndtr(mu)


def truncated_normal_right(mu):
    m, v, lz = truncated_normal_left(-np.asarray(mu, dtype=np.float64))
    return -m, v, lz


class Config:
    def __init__(self, alpha_0=1.0, beta_0=1.0, gamma_0=1.0, mu_0=0.0, reg_0=1.0, fit_w0=True, fit_linear=True):
        self.alpha_0, self.beta_0, self.gamma_0, self.mu_0, self.reg_0 = alpha_0, beta_0, gamma_0, mu_0, reg_0
        self.fit_w0, self.fit_linear = fit_w0, fit_linear


def update_e_and_var(X, w0, w0_var, w, w_var, V, V_var):
    """(score, e_var_sum) of the mean model (:715-833)"""
    X2 = X.multiply(X).tocsr()
    X3 = X2.multiply(X).tocsr()
    X4 = X2.multiply(X2).tocsr()
    e = w0 + X @ w
    var = w0_var * X.shape[0] + (X2 @ w_var).sum()
    for r in range(V.shape[1]):
        v, s = V[:, r], V_var[:, r]
        q, q_s = X @ v, X2 @ (v * v)
        x2s, x3sv, x4s2, x4sv2 = X2 @ s, X3 @ (s * v), X4 @ (s * s), X4 @ (s * v * v)
        e = e + 0.5 * (q * q - q_s)
        var += (q * q * x2s + 0.5 * x2s * x2s - 2 * x3sv * q - 0.5 * x4s2 + x4sv2).sum()
    return e, var


class VBRef:
    """state: w0, w0_var, w, w_var, V, V_var (V (D, K)), e, hyper-parameters as the reference names them"""

    def __init__(self, X, y, rank, group_index, task, cfg, w0, w, V, init_std, blocks=()):
        """blocks: (original_to_block, csr) pairs, the RelationBlocks in order (their columns follow X's)"""
        self.X = sps.csr_matrix(X, dtype=np.float64)
        self.Xt = self.X.T.tocsr()
        self.y = np.asarray(y, dtype=np.float64)
        self.N, self.D0 = self.X.shape
        self.blocks = []
        off = self.D0
        for mp, B in blocks:
            B = sps.csr_matrix(B, dtype=np.float64)
            mp = np.asarray(mp, dtype=np.int64)
            self.blocks.append((mp, B, B.T.tocsr(), np.bincount(mp, minlength=B.shape[0]).astype(np.float64), off))
            off += B.shape[1]
        self.D = off
        # the flattened design: only the score pass uses it (update_e_and_var :715-833 sums the block caches per train row,
        # which is this product)
        self.Xf = sps.hstack([self.X] + [B[mp] for mp, B, _, _, _ in self.blocks]).tocsr() if self.blocks else self.X
        self.K = rank
        self.gi = np.asarray(group_index, dtype=np.int64)
        self.G = int(self.gi.max()) + 1 if self.D else 0
        self.groups = [np.nonzero(self.gi == g)[0] for g in range(self.G)]
        self.task = task  # "regression" / "classification"
        self.cfg = cfg
        self.w0, self.w0_var = float(w0), 1.0
        self.w = np.array(w, dtype=np.float64)
        self.w_var = np.full(self.D, init_std * init_std)
        self.V = np.array(V, dtype=np.float64).reshape(self.D, rank)
        self.V_var = np.full((self.D, rank), init_std * init_std)
        G, K = self.G, self.K
        self.alpha, self.alpha_rate = 1.0, self.N * 0.5
        self.mu_w, self.mu_w_var = np.zeros(G), np.ones(G)
        self.lambda_w, self.lambda_w_rate = np.full(G, 1e-5), np.ones(G)
        self.mu_V, self.mu_V_var = np.zeros((G, K)), np.ones((G, K))
        self.lambda_V, self.lambda_V_rate = np.full((G, K), 1e-5), np.ones((G, K))
        self.elbos = []
        # initialize_e: e -= y for both tasks
        self.e, self.e_var_sum = update_e_and_var(self.Xf, self.w0, self.w0_var, self.w, self.w_var, self.V, self.V_var)
        self.e = self.e - self.y

    @staticmethod
    def _bcol(Bt, l):
        a, b = Bt.indptr[l], Bt.indptr[l + 1]
        return Bt.indices[a:b], Bt.data[a:b]

    def _col(self, j):
        a, b = self.Xt.indptr[j], self.Xt.indptr[j + 1]
        return self.Xt.indices[a:b], self.Xt.data[a:b]

    def _lambda_mu(self, theta, var, mu, mu_var, lam, lam_rate):
        c = self.cfg
        for g, f in enumerate(self.groups):
            beta = c.beta_0 + np.sum((theta[f] - mu[g]) ** 2 + mu_var[g] + var[f])
            lam[g] = (c.alpha_0 + len(f)) / beta
            lam_rate[g] = beta / 2
        for g, f in enumerate(self.groups):
            square = lam[g] * (c.gamma_0 + len(f))
            linear = (c.gamma_0 * c.mu_0 + theta[f].sum()) * lam[g]
            mu[g] = linear / square
            mu_var[g] = 1 / square

    def step_alpha(self):
        if self.task == "classification":
            self.alpha, self.alpha_rate = 1.0, 1.0
            return
        e_all = np.sum(self.e**2) + self.e_var_sum
        rate = (self.cfg.beta_0 + e_all) / 2
        self.alpha, self.alpha_rate = (self.cfg.alpha_0 + self.N) / 2 / rate, rate

    def step_w0(self):
        if not self.cfg.fit_w0:
            self.w0 = self.w0_var = 0.0
            return
        lin = self.alpha * np.sum(self.w0 - self.e)
        quad = self.alpha * self.N + self.cfg.reg_0
        new = lin / quad
        self.e = self.e + (new - self.w0)
        self.w0, self.w0_var = new, 1 / quad

    def step_w(self):
        self._lambda_mu(self.w, self.w_var, self.mu_w, self.mu_w_var, self.lambda_w, self.lambda_w_rate)
        if not self.cfg.fit_linear:
            self.w[:] = 0
            self.w_var[:] = 0
        self.sweep_w()

    def sweep_w(self):
        e = self.e
        for j in range(self.D0):
            rows, x = self._col(j)
            g = self.gi[j]
            e[rows] -= x * self.w[j]
            square = self.lambda_w[g] + self.alpha * np.sum(x * x)
            linear = -self.alpha * np.dot(x, e[rows]) + self.lambda_w[g] * self.mu_w[g]
            self.w[j] = linear / square
            self.w_var[j] = 1 / square
            e[rows] += x * self.w[j]
        # relation blocks (:388-447): un-sync the block's linear part into per-block-row residual sums, sweep the block's
        # columns over them, re-sync
        for mp, B, Bt, card, off in self.blocks:
            wb = self.w[off:off + B.shape[1]]
            q = B @ wb
            eb = np.bincount(mp, weights=e, minlength=B.shape[0])
            e -= q[mp]
            for l in range(B.shape[1]):
                i, x = self._bcol(Bt, l)
                g = self.gi[off + l]
                w_old = wb[l]
                square = np.sum(x * x * card[i])
                linear = -np.dot(x, eb[i]) + square * w_old
                square = self.lambda_w[g] + self.alpha * square
                linear = self.alpha * linear + self.lambda_w[g] * self.mu_w[g]
                wb[l] = linear / square
                self.w_var[off + l] = 1 / square
                eb[i] += x * card[i] * (wb[l] - w_old)
            e += (B @ wb)[mp]

    def step_V(self, factors=None):
        for r in range(self.K):
            self._lambda_mu(self.V[:, r], self.V_var[:, r], self.mu_V[:, r], self.mu_V_var[:, r], self.lambda_V[:, r],
                            self.lambda_V_rate[:, r])
        for r in range(self.K) if factors is None else factors:
            self.sweep_factor(r)

    def sweep_factor(self, r):
        e = self.e
        v, s = self.V[:, r], self.V_var[:, r]
        # the row caches with every block's contribution added through original_to_block (:452-503)
        X = self.Xf
        X2 = X.multiply(X).tocsr()
        q, x2s, x3sv = X @ v, X2 @ s, X2.multiply(X).tocsr() @ (s * v)
        for j in range(self.D0):
            rows, x = self._col(j)
            g = self.gi[j]
            v_old, s_old = v[j], s[j]
            h = x * (q[rows] - x * v_old)
            a2 = x2s[rows] - x * x * s_old
            a3 = x3sv[rows] - x * x * x * s_old * v_old
            sq = np.sum(h * h)
            lin = np.sum(-e[rows] * h) + sq * v_old - np.sum(h * a2 - x * a3)
            sq = (sq + np.sum(a2 * x * x)) * self.alpha + self.lambda_V[g, r]
            lin = lin * self.alpha + self.lambda_V[g, r] * self.mu_V[g, r]
            v_new, s_new = lin / sq, 1 / sq
            q[rows] += x * (v_new - v_old)
            e[rows] += h * (v_new - v_old)
            x2s[rows] += x * x * (s_new - s_old)
            x3sv[rows] += x * x * x * (s_new * v_new - s_old * v_old)
            v[j], s[j] = v_new, s_new
        # relation blocks (:557-710)
        for mp, B, Bt, card, off in self.blocks:
            nb = B.shape[0]
            vb, sb = v[off:off + B.shape[1]], s[off:off + B.shape[1]]
            B2 = B.multiply(B).tocsr()
            qb, x2sb, x3svb = B @ vb, B2 @ sb, B2.multiply(B).tocsr() @ (sb * vb)
            q_S = B2 @ (vb * vb)
            # un-sync: the other features' part of every train row, summed per block row
            q -= qb[mp]
            x2s -= x2sb[mp]
            x3sv -= x3svb[mp]
            c_ = np.bincount(mp, weights=q, minlength=nb)
            c_S = np.bincount(mp, weights=q * q, minlength=nb)
            eb = np.bincount(mp, weights=e, minlength=nb)
            e_q = np.bincount(mp, weights=e * q, minlength=nb)
            c_x2s = np.bincount(mp, weights=x2s, minlength=nb)
            c_x3sv = np.bincount(mp, weights=x3sv, minlength=nb)
            c_x2s_q = np.bincount(mp, weights=x2s * q, minlength=nb)
            e -= q * qb[mp] + 0.5 * qb[mp] * qb[mp] - 0.5 * q_S[mp]
            for l in range(B.shape[1]):
                i, x = self._bcol(Bt, l)
                g = self.gi[off + l]
                v_old, s_old = vb[l], sb[l]
                cd = card[i]
                x2 = x * x
                x2sb[i] -= x2 * s_old
                x3svb[i] -= x * x2 * v_old * s_old
                h_B = qb[i] - x * v_old
                sq = np.sum(x * x * (h_B * h_B * cd + 2 * c_[i] * h_B + c_S[i]))
                lin = np.sum((-eb[i] * h_B - e_q[i]) * x)
                sq_var = np.sum((c_x2s[i] + x2sb[i] * cd) * x * x)
                lin_var = np.sum((c_x2s_q[i] + x2sb[i] * c_[i] + c_x2s[i] * h_B + x2sb[i] * h_B * cd - c_x3sv[i]
                                  - x3svb[i] * cd) * x)
                lin += sq * v_old
                lin -= lin_var
                sq += sq_var
                sq = sq * self.alpha + self.lambda_V[g, r]
                lin = lin * self.alpha + self.lambda_V[g, r] * self.mu_V[g, r]
                v_new, s_new = lin / sq, 1 / sq
                delta = v_new - v_old
                vb[l], sb[l] = v_new, s_new
                qb[i] += delta * x
                q_S[i] += delta * (v_new + v_old) * x * x
                eb[i] += x * delta * (h_B * cd + c_[i])
                e_q[i] += x * delta * (h_B * c_[i] + c_S[i])
                x3svb[i] += x * x * x * v_new * s_new
                x2svb = x * x * s_new
                x2sb[i] += x2svb
            # re-sync
            e += q * qb[mp] + 0.5 * qb[mp] * qb[mp] - 0.5 * q_S[mp]
            q += qb[mp]
            x2s += x2sb[mp]
            x3sv += x3svb[mp]
        self.q, self.x2s, self.x3sv = q, x2s, x3sv

    def step_e(self):
        c = self.cfg
        score, self.e_var_sum = update_e_and_var(self.Xf,self.w0, self.w0_var, self.w, self.w_var, self.V, self.V_var)
        elbo = 0.0
        if self.task == "regression":
            self.e = score - self.y
        else:
            m_l, _, lz_l = truncated_normal_left(score)
            m_r, _, lz_r = truncated_normal_right(score)
            pos = self.y > 0
            m, lz = np.where(pos, m_l, m_r), np.where(pos, lz_l, lz_r)
            self.e = score - m
            elbo += np.sum(lz + (m - score) ** 2 / 2)
        elbo += -self.alpha * (c.beta_0 + np.sum(self.e**2) + self.e_var_sum) / 2
        elbo += self.alpha * self.alpha_rate * (1 - np.log(self.alpha_rate))
        with np.errstate(divide="ignore"):
            elbo += -c.gamma_0 * (self.w0 * self.w0 + self.w0_var) + 0.5 * np.log(self.w0_var)
        for g, f in enumerate(self.groups):
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

    def iterate(self):
        self.step_alpha()
        self.step_w0()
        self.step_w()
        self.step_V()
        self.step_e()

    def hyper(self):
        return dict(alpha=self.alpha, alpha_rate=self.alpha_rate, mu_w=self.mu_w, mu_w_var=self.mu_w_var, lambda_w=self.lambda_w,
                    lambda_w_rate=self.lambda_w_rate, mu_V=self.mu_V, mu_V_var=self.mu_V_var, lambda_V=self.lambda_V,
                    lambda_V_rate=self.lambda_V_rate)


def initial_weights(X, y, rank, init_std, seed, blocks=()):
    """the VB start (variational.hpp:70-89) from the CPU oracle's Gibbs start (FM.hpp:34-45): one stream, reassigned"""
    from oracle import oracle as O

    w0, w, V = O.OracleTrainer(X, y, blocks, rank=rank, init_std=init_std, seed=seed).fm()
    D = w.shape[0]
    s = np.concatenate([np.asarray(V).ravel("F"), np.asarray(w), [w0]])
    return s[0], s[1:1 + D], s[1 + D:].reshape((D, rank), order="F")
