"""The exact t-SNE contract of include/scde_hip.h restated in numpy, plainly vectorised.

Every function takes ``dtype`` (``numpy.float64`` or ``numpy.longdouble``) and an optional index
permutation ``perm``: the points are renumbered before the computation and numbered back after
it, so every sum over points is taken in another order while the mathematics stays the same.
Nothing here knows how the kernels tile or reduce.
"""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny
FLT_MIN = 2.0 ** -126
DEFAULTS = dict(eta=200.0, exaggeration=12.0, stop_lying_iter=250, mom_switch_iter=250, momentum=0.5,
                final_momentum=0.8)


def clusters(n, k, seed=0, dims=10):
    """Well-separated Gaussian clusters: k centres N(0, 4^2) in ``dims`` dimensions, unit
    noise, label i mod k.  (Euclidean distance matrix, labels)."""
    rng = np.random.default_rng([seed, n, k])
    centres = rng.normal(0.0, 4.0, (k, dims))
    lab = np.arange(n) % k
    x = centres[lab] + rng.normal(0.0, 1.0, (n, dims))
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return d, lab


def lower_d2(d, squared=False):
    """D2 from the strict lower triangle of d (symmetric, zero diagonal)."""
    low = np.tril(np.asarray(d, dtype=np.float64), -1)
    delta = low + low.T
    return delta if squared else delta * delta


def affinities(D2, perplexity, dtype=np.float64, perm=None):
    """(P, beta, evaluations per row, |delta| at each row's last evaluation)."""
    n = D2.shape[0]
    if perm is not None:
        inv = np.argsort(perm)
        P, beta, ev, dl = affinities(D2[np.ix_(perm, perm)], perplexity, dtype)
        return P[np.ix_(inv, inv)], beta[inv], ev[inv], dl[inv]
    T = dtype
    D2 = np.asarray(D2).astype(T)
    off = (~np.eye(n, dtype=bool)).astype(T)
    logp = np.log(T(perplexity))
    beta, lo, hi = np.ones(n, T), np.full(n, -np.inf, T), np.full(n, np.inf, T)
    s_last, d_last, evals = np.zeros(n, T), np.zeros(n, T), np.zeros(n, int)
    act = np.arange(n)
    for ev in range(200):
        b = beta[act]
        p = np.exp(-b[:, None] * D2[act]) * off[act]
        s = p.sum(1) + T(DBL_MIN)
        delta = b * (D2[act] * p).sum(1) / s + np.log(s) - logp
        s_last[act], d_last[act], evals[act] = s, delta, ev + 1
        go = ~(np.abs(delta) < T(1e-5))
        if ev == 199 or not go.any():
            break
        act, delta, b = act[go], delta[go], b[go]
        up = delta > 0
        lo[act] = np.where(up, b, lo[act])
        hi[act] = np.where(up, hi[act], b)
        beta[act] = np.where(up, np.where(np.isinf(hi[act]), b * T(2), (b + hi[act]) / T(2)),
                             np.where(np.isinf(lo[act]), b / T(2), (b + lo[act]) / T(2)))
    cond = np.exp(-beta[:, None] * D2) * off / s_last[:, None]
    return (cond + cond.T) / T(2 * n), beta, evals, np.abs(d_last)


def _sums(P, Y, ex, T):
    n = Y.shape[0]
    off = (~np.eye(n, dtype=bool)).astype(T)
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    Q = T(1) / (T(1) + dx * dx + dy * dy) * off
    W = (T(ex) * P) * Q
    A = np.stack([(W * dx).sum(1), (W * dy).sum(1)], 1)
    Q2 = Q * Q
    R = np.stack([(Q2 * dx).sum(1), (Q2 * dy).sum(1)], 1)
    return A, R, Q.sum(1), Q


def step(P, Y, uY, gains, t, dtype=np.float64, **kw):
    """Iteration t on (Y, uY, gains): the new (Y, uY, gains, dY)."""
    T = dtype
    prm = dict(DEFAULTS, **kw)
    ex = prm["exaggeration"] if t <= prm["stop_lying_iter"] else 1.0
    mom = prm["momentum"] if t <= prm["mom_switch_iter"] else prm["final_momentum"]
    n = Y.shape[0]
    A, R, S, _ = _sums(P, Y, ex, T)
    dY = A - R / S.sum()
    gains = np.where(np.sign(dY) != np.sign(uY), gains + T(0.2), gains * T(0.8))
    gains = np.maximum(gains, T(0.01))
    uY = T(mom) * uY - T(prm["eta"]) * gains * dY
    Y = Y + uY
    Y = Y - Y.sum(0) / T(n)
    return Y, uY, gains, dY


def iterate(P, Y, uY, gains, t0, n_iter, dtype=np.float64, perm=None, **kw):
    """Iterations t0 .. t0 + n_iter - 1: (Y, uY, gains)."""
    T = dtype
    P, Y, uY, gains = (np.asarray(x).astype(T) for x in (P, Y, uY, gains))
    if perm is not None:
        inv = np.argsort(perm)
        out = iterate(P[np.ix_(perm, perm)], Y[perm], uY[perm], gains[perm], t0, n_iter, dtype, **kw)
        return tuple(x[inv] for x in out)
    for t in range(t0, t0 + n_iter):
        Y, uY, gains, _ = step(P, Y, uY, gains, t, T, **kw)
    return Y, uY, gains


def start(Y0, dtype=np.float64):
    Y0 = np.asarray(Y0).astype(dtype)
    return Y0, np.zeros_like(Y0), np.ones_like(Y0)


def costs(P, Y, dtype=np.float64, perm=None):
    T = dtype
    P, Y = np.asarray(P).astype(T), np.asarray(Y).astype(T)
    if perm is not None:
        return costs(P[np.ix_(perm, perm)], Y[perm], dtype)[np.argsort(perm)]
    _, _, S, Q = _sums(P, Y, 1.0, T)
    off = ~np.eye(P.shape[0], dtype=bool)
    term = P * np.log((P + T(FLT_MIN)) / (Q / S.sum() + T(FLT_MIN)))
    return np.where(off, term, T(0)).sum(1)


def purity(Y, lab, k=5):
    """Mean share of each point's k nearest neighbours in Y that carry its label."""
    Y = np.asarray(Y, dtype=np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((lab[nn] == lab[:, None]).mean())
