"""Plain float64 numpy / scipy restatement of ``pagoda.top.aspects`` (R/functions.R:2000-2014,
2277-2456, 5096-5124) for the tests, written independently of ``scde_amd.top_aspects`` and
``scde_amd.rmt``: the Tracy-Widom law from ``eigvalsh`` of one Gauss-Legendre rule, quantiles from
scipy's root finders, Benjamini-Hochberg in linear space, the normal quantile through
``norm.isf(exp(lp))``.  It is only valid where those are (moderate tails); the deep tails are
checked against mpmath (``tw_upper_log_mp``, ``qnorm_upper_log_mp``).
"""
from __future__ import annotations

import math

import numpy as np
from scipy import optimize, stats
from scipy.special import airy, gammaincc

TW1_MEAN = -1.2065335745820
TW1_VAR = 1.607781034581
U = 2.0 ** -52          # ulp(1)


def bar(ref_err, scale=1.0):
    """The tolerance rule of tests/test_gpu_aspects.py: 16 x the float64 restatement's own maximum
    error on the case plus 8 ulp of the result's scale."""
    return 16.0 * ref_err + 8.0 * U * scale


# ------------------------------------------------------------------ Tracy-Widom, float64
def tw_log_cdf64(s, n=128):
    """log F1(s) = sum(log1p(-lambda)) of the Nystrom matrix of Ai((x + y) / 2) / 2 on n
    Gauss-Legendre nodes over (s, s + 24 + 2 max(0, -s)).  Good to 1e-12 for s >= -4."""
    length = 24.0 + 2.0 * max(0.0, -s)
    x, w = np.polynomial.legendre.leggauss(n)
    x = s + 0.5 * length * (x + 1.0)
    w = 0.5 * length * w
    sw = np.sqrt(w)
    k = 0.5 * airy(0.5 * (x[:, None] + x[None, :]))[0] * sw[:, None] * sw[None, :]
    return float(np.sum(np.log1p(-np.linalg.eigvalsh(k))))


def ptw_upper_log64(s):
    """log(1 - F1); -inf where the matrix has underflowed (s above 100), NaN where an eigenvalue
    has passed 1 (s below about -9)."""
    up = [-math.expm1(tw_log_cdf64(float(v))) for v in np.atleast_1d(s)]
    return np.array([math.log(v) if v > 0 else (-math.inf if v == 0 else math.nan) for v in up])


def qtw_upper64(p):
    return optimize.brentq(lambda s: ptw_upper_log64(s)[0] - math.log(p), -6.0, 40.0, xtol=1e-13, rtol=1e-13)


def wishart_par(ndf, pdim):
    a, b = np.sqrt(ndf - 0.5), np.sqrt(np.asarray(pdim, dtype=np.float64) - 0.5)
    return (a + b) ** 2 / ndf, (a + b) * np.cbrt(1.0 / a + 1.0 / b) / ndf


def r_tail(s):
    """R/functions.R:2303's formula, where gammaincc does not underflow."""
    return np.log(gammaincc(2.0 / 3.0, (2.0 / 3.0) * np.asarray(s) ** 1.5)) + math.lgamma(2.0 / 3.0) + math.log(
        (2.0 / 3.0) ** (1.0 / 3.0))


# ------------------------------------------------------------------ log-space helpers
def qnorm_upper_log64(lp):
    """qnorm(lp, lower.tail = FALSE, log.p = TRUE) where exp(lp) is a normal number."""
    lp = np.asarray(lp, dtype=np.float64)
    return stats.norm.isf(np.exp(lp))


def bh_linear(p):
    """bh.adjust(p) (R/functions.R:5111-5124), NaN skipped and kept; not capped at 1, as R's is not."""
    p = np.asarray(p, dtype=np.float64)
    out = p.copy()
    ok = np.nonzero(~np.isnan(p))[0]
    x = p[ok]
    o = np.argsort(x, kind="stable")
    q = x[o] * len(x) / np.arange(1, len(x) + 1)
    a = np.minimum.accumulate(q[::-1])[::-1]
    res = np.empty(len(x))
    res[o] = a
    out[ok] = res
    return out


def pgev_upper_log(x, loc, scale):
    """pgev.upper.log with shape 0."""
    t = np.minimum(0.0, -(np.asarray(x, dtype=np.float64) - loc) / scale)
    sw = (t > -5) & (t < 0)
    t[sw] = np.log(-np.expm1(-np.exp(t[sw])))
    return t


def gumbel_upper_quantile(p, loc, scale):
    return loc - scale * math.log(-math.log1p(-p))


# ------------------------------------------------------------------ pagoda.effective.cells
def effective_cells_fit(sn, sp):
    """vfit of R/functions.R:2008."""
    return (sn + sp) ** 2 / (sn * sn + 0.5) + TW1_MEAN * (sn + sp) * np.cbrt(1.0 / sn + 1.0 / sp) / (sn * sn + 0.5)


def effective_cells_objective(sn, v, sp):
    return float(np.sum((v - effective_cells_fit(sn, sp)) ** 2))


# ------------------------------------------------------------------ the table
def _rows(sets):
    """(i, var, n, npc, shz) of R/functions.R:2285-2290; sets: the non-None entries in order."""
    cols = {k: [] for k in ("i", "var", "n", "npc", "shz")}
    for i, x in enumerate(sets, start=1):
        v = np.asarray(x["sd"], dtype=np.float64).ravel() ** 2
        rv = x["xp"].get("randvar")
        shz = np.full(v.shape, np.nan) if rv is None else (v - np.mean(rv)) / np.std(rv, ddof=1)
        for k in range(len(v)):
            cols["i"].append(i)
            cols["var"].append(v[k])
            cols["n"].append(x["n"])
            cols["npc"].append(k + 1)
            cols["shz"].append(shz[k])
    return {k: np.array(v, dtype=np.float64) for k, v in cols.items()}


def _bh_z(z):
    return qnorm_upper_log64(np.log(bh_linear(stats.norm.sf(z))))


def table(pwpca, n_cells, clpca=None, gumbel=None, score_alpha=0.05, tail_from=None):
    """The merged table of R/functions.R:2285-2404 as {column: array}.  ``gumbel``: (location,
    scale) of the fit of clpca["varm"]["varst"]."""
    sets = [x for x in pwpca.values() if x is not None]
    t = _rows(sets)
    cen, sca = wishart_par(n_cells, t["n"])
    s = (t["var"] - cen) / sca
    lp = ptw_upper_log64(s)
    if tail_from is not None:
        lp[s >= tail_from] = r_tail(s[s >= tail_from])
    t["exp"] = cen + sca * qtw_upper64(0.5)
    t["z"] = qnorm_upper_log64(lp)
    t["cz"] = _bh_z(t["z"])
    t["ub"] = cen + sca * qtw_upper64(score_alpha / 2)
    t["ub_stringent"] = cen + sca * qtw_upper64(score_alpha / len(s) / 2)
    if clpca is not None:
        c = _rows(list(clpca["cl.goc"].values()))
        cen, sca = wishart_par(n_cells, c["n"])
        pm, pv = cen + TW1_MEAN * sca, TW1_VAR * sca
        co = clpca["clvlm"]["coefficients"]
        pvar = co["pm"] * pm + co["n"] * c["n"]
        loc, scale = gumbel
        varst = (c["var"] - pvar) / np.sqrt(pv)
        c["exp"] = loc * np.sqrt(pv) + pvar
        c["z"] = qnorm_upper_log64(pgev_upper_log(varst, loc, scale))
        c["cz"] = _bh_z(c["z"])
        c["ub"] = gumbel_upper_quantile(score_alpha / 2, loc, scale) * np.sqrt(pv) + pvar
        c["ub_stringent"] = gumbel_upper_quantile(score_alpha / 2 / len(varst), loc, scale) * np.sqrt(pv) + pvar
        c["i"] = c["i"] + len(sets)
        t = {k: np.concatenate([t[k], c[k]]) for k in t}
    t["adj_shz"] = _bh_z(t["shz"])
    t["score"] = t["var"] / t["exp"]
    t["oec"] = t["var"] / t["ub"]
    return t


# ------------------------------------------------------------------ the matrix step
def scale_rows(x, w, num, dtype=np.float64):
    """xv = (x - rowMeans(x)) * (num / sqrt(var(x))), xvw = w / rowSums(w), in ``dtype``."""
    x = np.asarray(x, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    num = np.asarray(num, dtype=dtype)
    c = x.shape[1]
    with np.errstate(all="ignore"):
        mean = x.sum(axis=1, dtype=dtype) / dtype(c)
        d = x - mean[:, None]
        var = (d * d).sum(axis=1, dtype=dtype) / dtype(c - 1)
        xv = d * (num / np.sqrt(var))[:, None]
        xvw = w / w.sum(axis=1, dtype=dtype)[:, None]
    return xv, xvw


# ------------------------------------------------------------------ mpmath
def _gauss_legendre_mp(mp, n):
    """Gauss-Legendre nodes and weights on (0, 1) at mp's precision (Newton from numpy's)."""
    x0, _ = np.polynomial.legendre.leggauss(n)
    xs, ws = [], []
    for v in x0:
        x = mp.mpf(float(v))
        for _ in range(8):
            pn, pm = mp.legendre(n, x), mp.legendre(n - 1, x)
            dp = n * (x * pn - pm) / (x * x - 1)
            x = x - pn / dp
        pn, pm = mp.legendre(n, x), mp.legendre(n - 1, x)
        dp = n * (x * pn - pm) / (x * x - 1)
        xs.append((x + 1) / 2)
        ws.append(1 / ((1 - x * x) * dp * dp))
    return xs, ws


class _AiryMp:
    """Ai(u) at mp's precision: mpmath's airyai (3 ms a call at 40 digits) only at the multiples
    of 1/2, with Ai' there; between them the Taylor series of y'' = x y about the nearest one,
    c[j + 2] = (a c[j] + c[j - 1]) / ((j + 1) (j + 2)).  |u - a| <= 1/4, so 64 terms fall below
    1e-60 of the leading one for a up to 100."""

    def __init__(self, mp):
        self.mp, self.series = mp, {}

    def __call__(self, u):
        mp = self.mp
        k = int(mp.nint(2 * u))
        a = mp.mpf(k) / 2
        c = self.series.get(k)
        if c is None:
            y0 = mp.airyai(a)
            c = [y0, mp.airyai(a, derivative=1), a * y0 / 2]
            for j in range(1, 62):
                c.append((a * c[j] + c[j - 1]) / ((j + 1) * (j + 2)))
            self.series[k] = c = c[::-1]
        return mp.polyval(c, u - a)


def tw_upper_log_mp(s, panels=10, p=16, dps=40):
    """log(1 - F1(s)) from the same determinant, det(I - K) of Ai((x + y) / 2) / 2 on (s, s + 24 +
    2 max(0, -s)), with ``panels`` x ``p`` Gauss-Legendre nodes (160), Ai, the nodes and the
    logarithms by mpmath at ``dps`` digits.  Equal panels leave (2 panels - 1) p (p + 1) / 2
    distinct arguments of Ai.  The elimination of I - K runs on the entries as integers scaled
    by 2^bits (numpy object arrays), bits chosen so that the largest entry has 200 of them: the
    tiny kernels of the right tail keep 60 significant digits, and it is some 30 times faster
    than on mpf's."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(dps):
        xi, om = _gauss_legendre_mp(mp, p)
        length = mp.mpf(24) + 2 * max(mp.mpf(0), -mp.mpf(s))
        h = length / panels
        sw = [mp.sqrt(h * o) for o in om]
        n = panels * p
        val = {}
        with mp.workdps(dps + 10):
            ai = _AiryMp(mp)
            for c in range(2 * panels - 1):
                for q in range(p):
                    for r in range(q, p):
                        val[c, q, r] = ai(mp.mpf(s) + (c + xi[q] + xi[r]) * h / 2) * sw[q] * sw[r] / 2
        big = max(abs(v) for v in val.values())
        bits = 200 - int(mp.floor(mp.log(big, 2)))
        one = 1 << bits
        tab = np.empty((2 * panels - 1, p, p), dtype=object)
        for (c, q, r), v in val.items():
            tab[c, q, r] = tab[c, r, q] = int(mp.floor(mp.ldexp(v, bits)))
        ab = np.arange(panels)
        M = tab[ab[:, None] + ab[None, :]].transpose(0, 2, 1, 3).reshape(n, n).copy()
        with mp.workprec(bits + 64):
            acc = mp.mpf(0)
            for k in range(n):
                mk = M[k, k]
                d = one - mk
                if d <= 0:
                    return 0.0
                acc += mp.log1p(mp.ldexp(mp.mpf(-mk), -bits))
                if k + 1 < n:
                    col = M[k + 1:, k]
                    fac = (col << bits) // d
                    M[k + 1:, k + 1:] += (col[:, None] * fac[None, :]) >> bits
            return float(mp.log(-mp.expm1(acc)))


def qnorm_upper_log_mp(lp, dps=40):
    """The z with log(1 - Phi(z)) = lp, by mpmath."""
    import mpmath
    mp = mpmath.mp
    with mp.workdps(dps):
        f = lambda z: mp.log(mp.erfc(z / mp.sqrt(2)) / 2) - mp.mpf(lp)  # noqa: E731
        return float(mp.findroot(f, mp.sqrt(-2 * mp.mpf(lp))))
