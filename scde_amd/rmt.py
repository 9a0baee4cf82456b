"""Host statistics of ``pagoda.gene.clusters``' null model (R/functions.R:2196-2211), plain numpy:
the Tracy-Widom centring and scaling of a white Wishart matrix's largest eigenvalue, the
regression of the sampled PC1 variances on it, and the Gumbel fit of the standardised residuals.

For ``pagoda.top.aspects`` (R/functions.R:2293-2323) it also evaluates the Tracy-Widom law
(beta = 1) itself, from its Fredholm determinant, where R reads RMTstat's tables:
``ptw_upper_log``, ``qtw_upper``, ``p_wishart_max_upper_log``, ``q_wishart_max_upper``.

Neither RMTstat nor extRemes was run against this module; what each function restates, and how far
that was checked, is in its docstring and in DESIGN.md sections 4.8 and 4.13.
"""
from __future__ import annotations

import numpy as np

# mean and variance of the Tracy-Widom law (beta = 1) as R/functions.R:2199-2200 spells them
TW1_MEAN = -1.2065335745820
TW1_VAR = 1.607781034581


def wishart_max_par(ndf, pdim):
    """``RMTstat::WishartMaxPar(ndf, pdim, var = 1, beta = 1)``: centring and scaling of the
    largest eigenvalue of a white Wishart matrix with ``ndf`` degrees of freedom and dimension
    ``pdim`` (scalars or arrays, broadcast)::

        m = (sqrt(ndf - 1/2) + sqrt(pdim - 1/2))^2
        s = (sqrt(ndf - 1/2) + sqrt(pdim - 1/2)) * (1/sqrt(ndf - 1/2) + 1/sqrt(pdim - 1/2))^(1/3)
        centering = m / ndf,  scaling = s / ndf

    RMTstat is not available here.  This is its published formula (Johnstone's centring and
    scaling with the -1/2 correction), not checked against the package."""
    ndf = np.asarray(ndf, dtype=np.float64)
    pdim = np.asarray(pdim, dtype=np.float64)
    if np.any(ndf < 1) or np.any(pdim < 1):
        raise ValueError("ndf and pdim must be at least 1")
    a, b = np.sqrt(ndf - 0.5), np.sqrt(pdim - 0.5)
    m = (a + b) ** 2
    s = (a + b) * np.cbrt(1.0 / a + 1.0 / b)
    return {"centering": m / ndf, "scaling": s / ndf}


def score_varm(varm, n_cells):
    """R/functions.R:2198-2208 on ``varm`` = {"n", "var", "round"} (equal-length arrays, rows in
    round order).  Returns ``(varm, clvlm, tci)``:

    * ``varm`` gains ``pm = centering - 1.2065335745820 scaling``, ``pv = 1.607781034581 scaling``
      (``wishart_max_par(n_cells, n)``) and ``varst = (var - fitted) / sqrt(pv)``;
    * ``clvlm``: the least-squares fit ``lm(var ~ 0 + pm + n)`` as {"coefficients": {"pm", "n"},
      "fitted.values", "residuals"};
    * ``tci``: per round, in increasing round number, the row of ``varm`` holding the round's first
      maximum of ``varst`` (``which.max``).  Rows are 0-based here; R's are 1-based."""
    n = np.asarray(varm["n"])
    var = np.asarray(varm["var"], dtype=np.float64)
    rnd = np.asarray(varm["round"])
    if not (n.ndim == var.ndim == rnd.ndim == 1 and len(n) == len(var) == len(rnd)):
        raise ValueError("varm needs n, var and round of one length")
    if len(n) < 2:
        raise ValueError("varm needs at least 2 rows")
    x = wishart_max_par(n_cells, n)
    pm = x["centering"] + TW1_MEAN * x["scaling"]
    pv = TW1_VAR * x["scaling"]
    design = np.column_stack([pm, n.astype(np.float64)])
    coef, _, rank, _ = np.linalg.lstsq(design, var, rcond=None)
    if rank < 2:
        raise ValueError("var ~ 0 + pm + n is rank deficient (every cluster has the same size)")
    fitted = design @ coef
    varst = (var - fitted) / np.sqrt(pv)
    out = dict(varm)
    out.update(n=n, var=var, round=rnd, pm=pm, pv=pv, varst=varst)
    clvlm = {"coefficients": {"pm": float(coef[0]), "n": float(coef[1])}, "fitted.values": fitted,
             "residuals": var - fitted}
    tci = {}
    for r in np.unique(rnd):
        rows = np.nonzero(rnd == r)[0]
        tci[int(r)] = int(rows[np.argmax(varst[rows])])  # argmax: the first maximum
    return out, clvlm, tci


def gumbel_fit(x):
    """Maximum-likelihood Gumbel (maxima) parameters {"location", "scale"}: what
    ``extRemes::fevd(x, type = "Gumbel")`` approximates with ``optim``, so R's numbers agree
    with these only to ``optim``'s tolerance.  The likelihood has one maximum; its scale solves

        sigma = mean(x) - sum(x exp(-x / sigma)) / sum(exp(-x / sigma))

    (exponentials shifted by min(x)), found by Newton steps kept inside a bracket (bisection
    when a step leaves it); then ``mu = -sigma log(mean(exp(-x / sigma)))``.  Fewer than three
    values, a constant sample or a non-finite value raise ``ValueError``."""
    x = np.asarray(x, dtype=np.float64).ravel()
    if x.size < 3:
        raise ValueError("gumbel_fit needs at least 3 values")
    if not np.all(np.isfinite(x)):
        raise ValueError("gumbel_fit needs finite values")
    x0 = x.min()
    z = x - x0
    if z.max() == 0.0:
        raise ValueError("gumbel_fit: the sample is constant")
    zbar = z.mean()

    def g(s):
        """(g, g') of g(s) = s - zbar + sum(z w) / sum(w), w = exp(-z / s); increasing in s."""
        w = np.exp(-z / s)
        sw, szw, szzw = w.sum(), (z * w).sum(), (z * z * w).sum()
        m1 = szw / sw
        return s - zbar + m1, 1.0 + (szzw / sw - m1 * m1) / (s * s)

    # g(s) -> -zbar < 0 as s -> 0 (the weights concentrate on the minimum); g(s) > 0 for large s
    lo, hi = 0.0, max(zbar, z.std())
    while g(hi)[0] <= 0.0:
        lo, hi = hi, 2.0 * hi
        if not np.isfinite(hi):
            raise ValueError("gumbel_fit: no bracket for the scale")
    s = 0.5 * (lo + hi)
    for _ in range(200):
        v, dv = g(s)
        if v > 0.0:
            hi = s
        else:
            lo = s
        step = s - v / dv
        new = step if lo < step < hi else 0.5 * (lo + hi)
        if new == s or hi - lo <= 4.0 * np.finfo(np.float64).eps * hi:
            s = new
            break
        s = new
    w = np.exp(-z / s)
    return {"location": float(x0 - s * np.log(w.mean())), "scale": float(s)}


# ================================================================== the Tracy-Widom law, beta = 1
# F1(s) = det(I - T_s), T_s(x, y) = Ai((x + y) / 2) / 2 on L2(s, inf) (Ferrari and Spohn), by
# Bornemann's method: the operator is replaced by its Nystrom matrix on a quadrature rule.
#
#   * The interval is (s, s + L), L = 24 + 2 max(0, -s): the kernel left out is below
#     Ai(12) / 2 = 3e-14, and its effect on the determinant is of second order.  (A fixed
#     length of 24 is enough from s = -4 upwards and is off by 1e-3 in log F1 at s = -8.)
#   * The rule is Gauss-Legendre with _TW_P nodes on each of ceil(L / 2.4) panels of equal width.
#     With equal panels the sums x_i + x_j of a pair of panels depend only on the sum of the
#     panels' numbers, so Ai is evaluated about a thousand times and not n^2 / 2 = 5,000 times.
#   * log F1 = sum(log1p(-m_k)) over the pivots 1 - m_k of the symmetric elimination of I - K,
#     carried as the matrix M with I - M the Schur complement, in np.longdouble.  Mathematically
#     this is sum(log1p(-lambda_i)) over K's eigenvalues; numerically it keeps the relative
#     accuracy of a tiny K (the right tail) and of pivots near 0 (the left tail), where
#     eigvalsh's absolute error of 1e-16 in an eigenvalue 1 - 1e-8 leaves six digits.  I - K is
#     positive definite while every eigenvalue is below 1, so no pivoting is needed; a pivot
#     that is not positive means an eigenvalue has reached 1 to working accuracy: F1 = 0.
#   * Below s = -5 the entries with arguments up to 3 take Ai from _airy_ld (np.longdouble);
#     above s = 40 the trace stands for the determinant (_tw_upper_log_far).
_TW_P = 10
_TW_LEFT = -16.0   # below this F1 < exp(-150) and the upper tail is 1 to 65 digits

_tw_rule_cache = {}


def _tw_rule():
    """The panel rule on (0, 1): nodes, weights and the upper-triangle index pairs."""
    if not _tw_rule_cache:
        from numpy.polynomial.legendre import leggauss
        ld = np.longdouble
        n = _TW_P
        x = leggauss(n)[0].astype(ld)
        for _ in range(3):   # Newton steps on P_n in np.longdouble (three-term recurrence)
            p0, p1 = np.ones_like(x), x
            for k in range(2, n + 1):
                p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
            dp = n * (x * p1 - p0) / (x * x - 1)
            x = x - p1 / dp
        p0, p1 = np.ones_like(x), x
        for k in range(2, n + 1):
            p0, p1 = p1, ((2 * k - 1) * x * p1 - (k - 1) * p0) / k
        dp = n * (x * p1 - p0) / (x * x - 1)
        om = 2 / ((1 - x * x) * dp * dp)
        _tw_rule_cache.update(xi=(x + 1) / 2, om=om / 2, tri=np.triu_indices(n))
    return _tw_rule_cache["xi"], _tw_rule_cache["om"], _tw_rule_cache["tri"]


_AI0 = "0.355028053887817239260063186004183"     # Ai(0) = 3^(-2/3) / Gamma(2/3)
_AIP0 = "-0.258819403792806798405183560189204"   # Ai'(0) = -3^(-1/3) / Gamma(1/3)
_AI_TERMS = 72
_AI_RIGHT = 3.0    # Taylor steps carry Ai up to here: their error grows like Bi, 1e-19 Bi(3) = 1.4e-18
_ai_series = {}


def _airy_ld(u):
    """Ai(u) in np.longdouble for -40 <= u <= _AI_RIGHT: the solution of y'' = x y carried from
    (Ai(0), Ai'(0)) to the anchors at the multiples of 1/2 by its Taylor series, c[j + 2] =
    (a c[j] + c[j - 1]) / ((j + 1) (j + 2)), and from the nearest anchor to u.  On the negative
    axis both solutions oscillate with the same amplitude, so the steps do not amplify rounding;
    to the right the error grows like Bi, which is why the steps stop at 3.  scipy's Ai is
    good to 1e-16 .. 9e-16 absolute around the origin, which pivots of 1e-8 (s = -8) turn into
    1e-8 in F1; this is good to 2e-18."""
    ld = np.longdouble
    nt = _AI_TERMS
    if not _ai_series:
        jj = np.arange(nt).astype(ld)
        for step, last in ((ld(-0.5), -80), (ld(0.5), int(2 * _AI_RIGHT))):
            y, dy = ld(_AI0), ld(_AIP0)
            pw = step ** jj
            for k in range(0, last + (1 if last > 0 else -1), 1 if last > 0 else -1):
                a = ld(k) / 2
                c = [y, dy, a * y / 2]
                for j in range(1, nt - 2):
                    c.append((a * c[j] + c[j - 1]) / ((j + 1) * (j + 2)))
                c = np.array(c, dtype=ld)
                _ai_series[k] = c
                y, dy = np.sum((c * pw)[::-1]), np.sum((c[1:] * jj[1:] * pw[:-1])[::-1])
    u = np.asarray(u, dtype=ld)
    k = np.clip(np.rint(2 * u).astype(np.int64), -80, int(2 * _AI_RIGHT))
    d = u - k.astype(ld) / 2
    out = np.zeros(u.shape, dtype=ld)
    for kk in np.unique(k):
        sel = k == kk
        c, dd = _ai_series[int(kk)], d[sel]
        acc = np.full(dd.shape, c[-1])
        for j in range(nt - 2, -1, -1):
            acc = acc * dd + c[j]
        out[sel] = acc
    return out


def _tw_log_cdf(s):
    """log F1(s) of one finite s as np.longdouble; -inf where F1 is 0 to working accuracy."""
    from scipy.special import airy
    if s < _TW_LEFT:
        return np.longdouble(-np.inf)
    xi, om, (iq, ir) = _tw_rule()
    length = 24.0 + 2.0 * max(0.0, -s)
    m = int(np.ceil(length / 2.4))
    p = _TW_P
    # Ai at s + (c + xi_q + xi_r) h / 2, c = the sum of two panel numbers, q <= r
    # The arguments are formed in np.longdouble; Ai is scipy's at the nearest double plus Ai'
    # times the remainder, so the rounding of an argument (3e-15 at 30, times Ai' of order 1)
    # does not enter: near the left end these entries decide pivots of 1e-8.
    ld = np.longdouble
    h = ld(length) / m
    c = np.arange(2 * m - 1).astype(ld)
    u = ld(s) + (c[:, None] + (xi[iq] + xi[ir])[None, :]) * (h / 2)
    ud = u.astype(np.float64)
    ai, aip = airy(ud)[:2]
    tri = ai.astype(ld) + (u - ud.astype(ld)) * aip.astype(ld)
    if s < -5.0:   # (from here down the entries around the origin need more than scipy's Ai holds)
        near = u <= _AI_RIGHT
        tri[near] = _airy_ld(u[near])
    tab = np.empty((2 * m - 1, p, p), dtype=ld)
    tab[:, iq, ir] = tri
    tab[:, ir, iq] = tri
    sw = np.sqrt(h * om)
    tab *= sw[:, None] * sw[None, :] / 2
    ab = np.arange(m)
    n = m * p
    M = tab[ab[:, None] + ab[None, :]].transpose(0, 2, 1, 3).reshape(n, n).copy()
    acc = np.longdouble(0.0)
    for k in range(n):
        mk = M[k, k]
        d = 1 - mk
        if not d > 0:
            return np.longdouble(-np.inf)
        acc += np.log1p(-mk)
        if k + 1 < n:
            col = M[k + 1:, k]
            M[k + 1:, k + 1:] += col[:, None] * (col / d)[None, :]
    return acc


_TW_FAR = 40.0


def _tw_upper_log_far(s):
    """log(1 - F1(s)) for s > _TW_FAR.  1 - det(I - T_s) = tr T_s - ..., and the terms after the
    trace are of relative size exp(-(2/3) s^1.5) < 1e-73 here, so this is log of tr T_s =
    (1/2) int_s^inf Ai: with zeta(x) = (2/3) x^1.5 and scipy's scaled ``airye`` = Ai exp(zeta),

        -zeta(s) + log((1/2) int_0^T airye(s + t) exp(-(zeta(s + t) - zeta(s))) dt),  T = 45 / sqrt(s),

    the integrand falling like exp(-sqrt(s) t), by a 48-point Gauss-Legendre rule.  The matrix
    of the determinant underflows from s = 104 on; a strong gene set reaches several hundred."""
    from numpy.polynomial.legendre import leggauss
    from scipy.special import airye
    s = np.float64(s)
    with np.errstate(over="ignore"):
        zeta = (2.0 / 3.0) * s ** 1.5
    if not np.isfinite(zeta):
        return -np.inf
    x, w = leggauss(48)
    half = 22.5 / np.sqrt(s)
    t = half * (x + 1.0)
    dz = (2.0 / 3.0) * (s + t) ** 1.5 - zeta
    return float(-zeta + np.log(0.5 * np.sum(half * w * airye(s + t)[0] * np.exp(-dz))))


def ptw_upper_log(s):
    """log(1 - F1(s)), the log upper tail of the Tracy-Widom law (beta = 1), for a scalar or an
    array: ``RMTstat::ptw(s, beta = 1, lower.tail = FALSE, log.p = TRUE)`` evaluated from the
    Fredholm determinant (see above) as ``log(-expm1(log F1))`` -- ``log1p(-exp(log F1))`` where
    F1 is below 1/2 -- so it keeps relative accuracy far into the right tail (-24.79 at s = 10,
    -114.06 at s = 30) and for a small F1 on the left.  Where F1 is 0 to working accuracy (a
    pivot that is not positive; with 64-bit long doubles only) and for s < -16 (F1 < 1e-65) the
    result is 0; s = +inf gives -inf, s = -inf 0, NaN NaN.  Above s = 40 the determinant's
    first-order term, the trace, stands for it (``_tw_upper_log_far``; the rest is below 1e-73
    relative), so a set hundreds of scalings above the centre keeps a finite log tail.

    Against a 40-digit evaluation of the same determinant the relative error is below 1e-9 on
    [-8, 30] (DESIGN.md section 4.13 has the figures).  RMTstat's tables were not compared."""
    sa = np.asarray(s, dtype=np.float64)
    out = np.empty(sa.shape)
    flat = out.reshape(-1)
    for j, v in enumerate(sa.reshape(-1)):
        if np.isnan(v):
            flat[j] = np.nan
        elif v == np.inf:
            flat[j] = -np.inf
        elif v > _TW_FAR:
            flat[j] = _tw_upper_log_far(float(v))
        else:
            lf = _tw_log_cdf(float(v))
            with np.errstate(divide="ignore"):
                if lf > -0.6931471805599453:
                    flat[j] = float(np.log(-np.expm1(lf)))
                else:   # (F1 below 1/2: log(1 - F1) from log1p keeps the relative accuracy of a small F1)
                    flat[j] = float(np.log1p(-np.exp(lf))) if lf > -np.inf else 0.0
    return out if out.ndim else float(out)


def qtw_upper(p, log_p=False):
    """The s with upper tail probability p (``RMTstat::qtw(p, beta = 1, lower.tail = FALSE)``):
    a bracketed root (Brent) of ``ptw_upper_log(s) - log(p)`` to 1e-12 relative.  ``log_p``: p
    is a log probability.  p = 1 gives -inf and p = 0 +inf; scalars only."""
    from scipy.optimize import brentq
    lp = float(p) if log_p else (float(np.log(p)) if p > 0 else -np.inf)
    if np.isnan(lp) or lp > 0:
        raise ValueError("qtw_upper: p must be a probability")
    if lp == 0:
        return -np.inf
    if lp == -np.inf:
        return np.inf
    if lp in _qtw_cache:
        return _qtw_cache[lp]
    if len(_qtw_cache) > 256:
        _qtw_cache.clear()
    _qtw_cache[lp] = out = _qtw_root(lp)
    return out


_qtw_cache = {}   # (a root costs some fifteen evaluations of the law; the table asks for the same three again)


def _qtw_root(lp):
    from scipy.optimize import brentq
    f = lambda s: ptw_upper_log(s) - lp  # noqa: E731
    lo, hi = -12.0, 4.0
    while f(lo) <= 0:   # (ptw_upper_log is 0 below about -13: a p this close to 1 has no root above)
        lo -= 2.0
        if lo < _TW_LEFT - 2.0:
            return -np.inf
    while f(hi) >= 0:
        lo, hi = hi, 2.0 * hi
        if hi > 1e4:
            return np.inf
    return float(brentq(f, lo, hi, xtol=1e-13, rtol=1e-12, maxiter=200))


def _log_upper_gamma(a, x):
    """log Gamma(a, x), the unnormalised upper incomplete gamma function, x > 0: from
    ``gammaincc`` where that is a normal number, beyond it from Legendre's continued fraction
    (modified Lentz), which converges in a few steps there."""
    from scipy.special import gammaincc, gammaln
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        q = gammaincc(a, x)
        out = np.log(q) + gammaln(a)
    deep = (q < 1e-290) & (x > a + 1.0) & np.isfinite(x)
    if deep.any():
        xd = x[deep]
        tiny = 1e-300
        b = xd + 1.0 - a
        cc = np.full(xd.shape, 1.0 / tiny)
        d = 1.0 / b
        hh = d.copy()
        for i in range(1, 500):
            an = -i * (i - a)
            b = b + 2.0
            d = an * d + b
            d = np.where(np.abs(d) < tiny, tiny, d)
            cc = b + an / cc
            cc = np.where(np.abs(cc) < tiny, tiny, cc)
            d = 1.0 / d
            delta = d * cc
            hh = hh * delta
            if np.all(np.abs(delta - 1.0) < 1e-16):
                break
        out[deep] = -xd + a * np.log(xd) + np.log(hh)
    out[x == np.inf] = -np.inf
    return out


def r_tw_tail_log(s):
    """The right-tail formula R/functions.R:2303 puts where RMTstat's table gives -Inf::

        pgamma((2/3) s^(3/2), 2/3, lower.tail = FALSE, log.p = TRUE) + lgamma(2/3) + log((2/3)^(1/3))

    for s > 0 (NaN elsewhere).  It lies about 2.5 above the law's log upper tail (-16.15
    against -18.64 at s = 8)."""
    s = np.asarray(s, dtype=np.float64)
    out = np.full(s.shape, np.nan)
    ok = s > 0
    out[ok] = _log_upper_gamma(2.0 / 3.0, (2.0 / 3.0) * s[ok] ** 1.5) + np.log((2.0 / 3.0) ** (1.0 / 3.0))
    return out


def p_wishart_max_upper_log(q, ndf, pdim, tail_from=None):
    """log P(largest eigenvalue > q) of a white Wishart matrix (``wishart_max_par(ndf, pdim)``,
    var = 1, beta = 1) in the Tracy-Widom approximation: ``ptw_upper_log((q - centering) /
    scaling)``; q, ndf and pdim broadcast.  This is ``pWishartMaxFixed(q, ndf, pdim, lower.tail =
    FALSE)`` of R/functions.R:2299-2305 with one deviation: R takes ``r_tw_tail_log`` wherever
    RMTstat's table has run out (returns -Inf), and where that happens is not known here, so by
    default the law's own tail is used everywhere.  ``tail_from``: a value of the scaled
    statistic from which (>=) R's formula is used instead, for a caller who knows RMTstat's
    switch point."""
    q = np.asarray(q, dtype=np.float64)
    par = wishart_max_par(ndf, pdim)
    s = (q - par["centering"]) / par["scaling"]
    out = np.asarray(ptw_upper_log(s), dtype=np.float64)
    if tail_from is not None:
        sw = s >= float(tail_from)
        if sw.any():
            out = np.array(out, copy=True)
            out[sw] = r_tw_tail_log(s[sw])
    return out if out.ndim else float(out)


def q_wishart_max_upper(p, ndf, pdim):
    """``RMTstat::qWishartMax(p, ndf, pdim, var = 1, beta = 1, lower.tail = FALSE)``:
    ``centering + scaling * qtw_upper(p)`` (p a scalar; ndf and pdim broadcast)."""
    par = wishart_max_par(ndf, pdim)
    out = par["centering"] + par["scaling"] * qtw_upper(p)
    return out if np.ndim(out) else float(out)
