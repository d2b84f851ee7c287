"""The fold-in chain of the probit tasks (csrc/mfm_foldin_gibbs.hpp) restated on the host: the reference of
tests/test_gpu_fold_in_gibbs.py, proved in tests/test_fold_in_gibbs_cpu.py. Built on tests/fold_in_ref.py (problems, grouping, z
and f, the longdouble Cholesky factorisation and solves) and tests/philox_ref.py (the per-row streams and the truncated-normal
samplers, draw for draw).

Under kept sample s, Lambda = diag(lambda) + sum_i z_i z_i^T = L L^T is fixed (noise precision 1). From theta^0 = mu, sweep t:

    m_i = f_i + z_i^T theta^t
    d_i = truncated standard normal on the stream (seed, FOLDIN_LATENT_TAG + t, row = s n + i), i the grouped row:
            classifier:      y_i > 0: tn_left(-m_i), else tn_right(-m_i)
            ordered probit:  class 0: tn_right(g_0 - m_i); class C - 1: tn_left(g_{C-2} - m_i); else tn_twoside(g_{c-1} - m_i, g_c - m_i)
    r_i = z_i^T theta^t + d_i,   b = lambda mu + sum_i z_i r_i,   thetabar^{t+1} = Lambda^-1 b,   theta^{t+1} = thetabar^{t+1} + L^-T eps^t

with eps^t_j the Box-Muller value of counter word j >> 1 of the stream (seed, FOLDIN_DRAW_TAG + 1 + t, row = s U + u). `chain` runs
(= `view` of `run`: a run of T sweeps holds every shorter chain) this for every (sample, entity) at once with the linear algebra in `dtype` (np.longdouble: the reference; np.float64: the twin)
and the draws in float64 from the bound rounded to float64. It returns the last state, the mean of thetabar over the sweeps
t >= n_burn, cond_2(Lambda) and the chain's margin: the minimum over the cell's rows and sweeps of the samplers' own margins, of
|bound| for every one-sided draw (tn_left changes proposal at bound = 0) and of the distance of a two-sided bound from 0. A cell
with a small margin may take another path on a device whose bound differs in the last bits; callers leave it out and count it.
"""
import numpy as np

from tests import fold_in_ref as fr
from tests import philox_ref as ph

LD = np.longdouble
FOLDIN_DRAW_TAG = fr.FOLDIN_DRAW_TAG
FOLDIN_LATENT_TAG = 0x464F4C444C540000  # csrc/mfm_foldin_gibbs.hpp ("FOLDLT" << 16)
MAX_SWEEPS = 65535


def problem(rng, D, K, S, U, n_class=0, counts=None, scale=0.5):
    """fold_in_ref.problem with probit labels: n_class = 0 the classifier (y = +-1), else class indices in [0, n_class) and per
    sample the cutpoints `cut` (S, n_class - 1), the first near the middle of the scores and the gaps from [0.3, 1.2]"""
    p = fr.problem(rng, D, K, S, U, scale=scale, counts=counts)
    n = p["y"].shape[0]
    p["n_class"] = n_class
    if n_class == 0:
        p["y"] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        p["cut"] = None
    else:
        p["y"] = rng.integers(0, n_class, size=n).astype(np.float64)
        gaps = rng.uniform(0.3, 1.2, size=(S, n_class - 1))
        gaps[:, 0] = rng.normal(size=S) * 0.3 - 0.5 * gaps[:, 1:].sum(axis=1)
        p["cut"] = np.cumsum(gaps, axis=1)
    del p["alpha"]
    return p


def normals_of_rows(seed, word, rows, M):
    """eps (len(rows), M): component j is the Box-Muller value of counter word j >> 1 of the stream (seed, word, row), r cos for
    even j and r sin for odd j"""
    g = ph.RowRng(seed, word, np.asarray(rows, dtype=np.int64))
    eps = np.zeros((g.row.shape[0], M + 1))
    for n in range((M + 1) // 2):
        ux, uy = g.next2(n)
        r = np.sqrt(-2.0 * np.log(ux))
        s, c = ph.sincospi2(uy)
        eps[:, 2 * n], eps[:, 2 * n + 1] = r * c, r * s
    return eps[:, :M]


def normals(seed, word, S, U, M):
    """eps (S, U, M) of draw word `word`: fold_in_ref.normals on another word of the same streams, row = s U + u"""
    rows = (np.arange(S, dtype=np.int64)[:, None] * U + np.arange(U, dtype=np.int64)[None, :]).ravel()
    return normals_of_rows(seed, word, rows, M).reshape(S, U, M)


def latent_draws(p, m, t, seed):
    """(d (S, n), margin (S, n)): the sweep's truncated normals around the row means m (S, n) (grouped rows), float64"""
    S, n = m.shape
    rows = (np.arange(S, dtype=np.int64)[:, None] * n + np.arange(n, dtype=np.int64)[None, :]).ravel()
    g = ph.RowRng(seed, FOLDIN_LATENT_TAG + t, rows)
    y = np.broadcast_to(p["yg"], (S, n)).ravel()
    mm = m.ravel()
    d, margin = np.empty(S * n), np.empty(S * n)
    if p["n_class"] == 0:
        bound = np.asarray(LD(0) - mm if mm.dtype == LD else 0.0 - mm, dtype=np.float64)
        pos = np.flatnonzero(y > 0)
        neg = np.flatnonzero(~(y > 0))
        d[pos], margin[pos] = ph.tn_left(g.subset(pos), bound[pos])
        d[neg], margin[neg] = ph.tn_right(g.subset(neg), bound[neg])
        return d.reshape(S, n), np.minimum(margin, np.abs(bound)).reshape(S, n)
    C = p["n_class"]
    cls = y.astype(np.int64)
    cut = p["cut"].astype(mm.dtype)  # (S, C - 1)
    srow = np.repeat(np.arange(S), n)
    lo = np.asarray(cut[srow, np.maximum(cls - 1, 0)] - mm, dtype=np.float64)
    hi = np.asarray(cut[srow, np.minimum(cls, C - 2)] - mm, dtype=np.float64)
    first, last = np.flatnonzero(cls == 0), np.flatnonzero(cls == C - 1)
    mid = np.flatnonzero((cls > 0) & (cls < C - 1))
    d[first], margin[first] = ph.tn_right(g.subset(first), hi[first])
    margin[first] = np.minimum(margin[first], np.abs(hi[first]))
    d[last], margin[last] = ph.tn_left(g.subset(last), lo[last])
    margin[last] = np.minimum(margin[last], np.abs(lo[last]))
    d[mid], margin[mid] = ph.tn_twoside(g.subset(mid), lo[mid], hi[mid])
    margin[mid] = np.minimum(margin[mid], np.minimum(np.abs(lo[mid]), np.abs(hi[mid])))
    return d.reshape(S, n), margin.reshape(S, n)


def z_and_f(sample, X, dtype=LD):
    """(z (n, K + 1), f (n,)) of the rows of X under one sample (fold_in_ref.z_and_residual with y = 0: r = -f exactly)"""
    z, r = fr.z_and_residual(sample, X, np.zeros(X.shape[0]), dtype)
    return z, -r


def run(p, fit_linear, T, seed, dtype=LD):
    """T sweeps of every (sample, entity): dict(thetas, bars, eps (T, S, U, M): theta^{t+1}, thetabar^{t+1} and eps^t; margins
    (T, S, U): the margin of sweeps 0 .. t; cond (S, U), mu, lam (S, M), counts (U,))"""
    S, U, K = p["S"], p["U"], p["K"]
    o = 0 if fit_linear else 1
    M = K + 1 - o
    assert 1 <= T <= MAX_SWEEPS
    Xg, yg, off = fr.grouped(p["X"], p["y"], p["entity"], U)
    p = dict(p, yg=yg)
    n = Xg.shape[0]
    counts = np.diff(off)
    mu, lam = p["mu"][:, o:].astype(dtype), p["lam"][:, o:].astype(dtype)
    out = dict(mu=mu, lam=lam, counts=counts, margins=np.full((T, S, U), np.inf), cond=np.ones((S, U)),
               thetas=np.zeros((T, S, U, M), dtype=dtype), bars=np.zeros((T, S, U, M), dtype=dtype), eps=np.zeros((T, S, U, M)))
    if M == 0:
        return out
    z = np.empty((S, n, M), dtype=dtype)
    f = np.empty((S, n), dtype=dtype)
    for s in range(S):
        zs, f[s] = z_and_f(p["samples"][s], Xg, dtype)
        z[s] = zs[:, o:]
    Lam = np.zeros((S, U, M, M), dtype=dtype)
    for u in range(U):
        zu = z[:, off[u]:off[u + 1]]
        Lam[:, u] = np.einsum("sni,snj->sij", zu, zu)
        Lam[:, u, np.arange(M), np.arange(M)] += lam
    out["cond"] = np.linalg.cond(Lam.astype(np.float64))
    L = fr.cholesky_ld(Lam) if dtype == LD else np.linalg.cholesky(Lam)
    ent = np.repeat(np.arange(U), counts)
    theta = np.broadcast_to(mu[:, None, :], (S, U, M)).copy()
    margin = np.full((S, U), np.inf)
    for t in range(T):
        zt = (z * theta[:, ent]).sum(axis=-1)  # (S, n)
        d, mg = latent_draws(p, f + zt, t, seed)
        r = zt + d.astype(dtype)
        b = np.broadcast_to((lam * mu)[:, None, :], (S, U, M)).copy()
        for u in range(U):
            if counts[u]:
                sl = slice(off[u], off[u + 1])
                b[:, u] += np.einsum("snm,sn->sm", z[:, sl], r[:, sl])
                margin[:, u] = np.minimum(margin[:, u], mg[:, sl].min(axis=1))
        eps = normals(seed, FOLDIN_DRAW_TAG + 1 + t, S, U, M)
        yv = fr.solve_lower(L, b)
        theta = fr.solve_upper_t(L, yv + eps.astype(dtype))
        out["thetas"][t], out["bars"][t], out["eps"][t], out["margins"][t] = theta, fr.solve_upper_t(L, yv), eps, margin
    return out


def view(r, n_burn, n_inner):
    """the chain of n_burn + n_inner sweeps read off a run of at least as many: dict(last, mean (S, U, M), cond, margin (S, U), mu,
    lam (S, M), counts (U,)). last: theta after the last sweep; mean: (sum of thetabar over the sweeps t >= n_burn) / n_inner, added in
    sweep order. An entity without rows: mu bit for bit, and mu_j + eps^{T-1}_j / sqrt(lambda_j)."""
    T = n_burn + n_inner
    assert n_inner >= 1 and n_burn >= 0 and T <= r["thetas"].shape[0]
    dtype = r["thetas"].dtype.type
    mean = np.zeros(r["thetas"].shape[1:], dtype=dtype)
    for t in range(n_burn, T):
        mean += r["bars"][t]
    mean /= dtype(n_inner)
    last = r["thetas"][T - 1].copy()
    empty = r["counts"] == 0
    if last.shape[-1]:
        mean[:, empty] = r["mu"][:, None, :]
        last[:, empty] = r["mu"][:, None, :] + r["eps"][T - 1][:, empty].astype(dtype) / np.sqrt(r["lam"])[:, None, :]
    return dict(last=last, mean=mean, cond=r["cond"], margin=r["margins"][T - 1], mu=r["mu"], lam=r["lam"], counts=r["counts"])


def chain(p, fit_linear, n_burn, n_inner, seed, dtype=LD):
    return view(run(p, fit_linear, n_burn + n_inner, seed, dtype), n_burn, n_inner)


def tolerance(ref, theta, T):
    """(S, U): 16 T (M + n_u) 2^-52 cond_2(Lambda_ref) max(|theta_ref|_inf, |mu|_inf): fold_in_ref.tolerance's bound of one solve,
    once per sweep (the chain contracts, so a sweep's error does not outgrow its own bound)"""
    theta = np.asarray(theta, dtype=np.float64)
    M = theta.shape[-1]
    if M == 0:
        return np.zeros(theta.shape[:2])
    scale = np.maximum(np.abs(theta).max(axis=-1), np.abs(ref["mu"].astype(np.float64)).max(axis=-1)[:, None])
    return 16.0 * T * (M + ref["counts"][None, :]) * 2.0 ** -52 * ref["cond"] * scale


def quadrature_mean(p, grid=20001, width=12.0):
    """the posterior mean of theta = w_u of a rank-0 problem with one entity and one sample, on a grid: the prior N(mu, 1 / lambda)
    times the probit likelihood of every row"""
    from scipy.special import log_ndtr, ndtr

    Xg, yg, _ = fr.grouped(p["X"], p["y"], p["entity"], 1)
    _, f = z_and_f(p["samples"][0], Xg, np.float64)
    mu, lam = p["mu"][0, 0], p["lam"][0, 0]
    th = mu + np.linspace(-width, width, grid) / np.sqrt(lam)
    m = f[None, :] + th[:, None]
    if p["n_class"] == 0:
        ll = log_ndtr(np.where(yg > 0, m, -m)).sum(axis=1)
    else:
        cut = np.concatenate([[-np.inf], p["cut"][0], [np.inf]])
        cls = yg.astype(np.int64)
        with np.errstate(divide="ignore"):  # (the far ends of the grid: log 0 = -inf, weight 0)
            ll = np.log(ndtr(cut[cls + 1][None, :] - m) - ndtr(cut[cls][None, :] - m)).sum(axis=1)
    lp = ll - 0.5 * lam * (th - mu) ** 2
    wgt = np.exp(lp - lp.max())
    return float((wgt * th).sum() / wgt.sum())
