"""pagoda.varnorm (R/functions.R:1347-1811) and pagoda.subtract.aspect (1850-1862).

The stages of ``pagoda_varnorm``:

  1. weights   ``scde_pagoda_varnorm_weights_dev``: posteriors, modes, matw / bmatw (1414-1507);
               they stay in HBM for stages 2 and 4
  2. moments   ``k_varnorm_moments``: edf, wvar, rowSums(matw) and the batch versions (1511-1619)
  3. host      N-vectors only (numpy + scipy): the cv2 ~ magnitude trend, zval, the chi-squared
               map to the adjusted variance arv (1620-1706)
  4. matrix    ``k_varnorm_matrix``: the normalised matrix mat and its weights (1725-1804)

What differs from the reference, on purpose:

  * ``predict(scde.edff, ...)`` is the natural cubic spline through the 1,000 stored points of
    that gam (``load_edf_table``; the fixture is tests/golden/scde_edff.npz).  A 1-D thin-plate
    smooth is a natural cubic spline whose knots are its data, so this is the gam's own curve.
  * The trend ``mgcv::gam(cv2 ~ s(lev, k = smooth.df))`` (1630) is NOT reproduced.  mgcv builds
    its thin-plate basis from a seeded subsample and picks the smoothing parameter with its
    own optimiser; ``fit_trend`` is a weighted penalised natural cubic regression spline with
    GCV instead.  Results agree with R only as far as the two smoothers do, and that distance
    is unknown: nothing here was checked against R or mgcv.  A caller who has mgcv's
    predictions passes them as ``trend=``; everything else follows the reference's text.
  * ``minimize_underdispersion`` with ``fit_genes``: the reference multiplies a vector over the
    valid genes with one over the fitted genes (R recycles); here both are over the fitted genes.
  * ``gene_length`` (the second smooth) is not built.
"""
from __future__ import annotations

import numpy as np

from . import api
from ._lib import ScdeError, check, lib
from .api import _p
from .models import as_model_dict, model_matrix


# ================================================================== the edf table
class EdfTable:
    """log(edf) over a uniform grid of log(theta) with the second derivatives of the natural
    cubic spline through it (float64, computed once on the host)."""

    def __init__(self, lt, log_edf):
        from scipy.linalg import solve_banded
        lt = np.ascontiguousarray(lt, np.float64)
        y = np.ascontiguousarray(log_edf, np.float64)
        n = lt.size
        if lt.ndim != 1 or y.shape != lt.shape or n < 3:
            raise ValueError("edf table: lt and log_edf must be vectors of the same length >= 3")
        h = (lt[-1] - lt[0]) / (n - 1)
        if not h > 0 or np.max(np.abs(np.diff(lt) - h)) > 1e-9 * h:
            raise ValueError("edf table: lt must be an increasing uniform grid")
        if not (np.all(np.isfinite(lt)) and np.all(np.isfinite(y))):
            raise ValueError("edf table: non-finite entries")
        # natural spline: m[0] = m[n-1] = 0; h/6 m[i-1] + 2h/3 m[i] + h/6 m[i+1] = (y[i+1] - 2 y[i] + y[i-1]) / h
        ab = np.zeros((3, n - 2))
        ab[0, 1:] = h / 6.0
        ab[1, :] = 2.0 * h / 3.0
        ab[2, :-1] = h / 6.0
        m = np.zeros(n)
        m[1:-1] = solve_banded((1, 1), ab, (y[2:] - 2.0 * y[1:-1] + y[:-2]) / h)
        self.lt, self.log_edf, self.m2 = lt, y, m
        self.n, self.lt0, self.h = n, float(lt[0]), float(h)
        self.table = np.ascontiguousarray(np.concatenate([y, m]))

    def log_edf_at(self, x):
        """S(x): the spline at log(theta) = x (linear beyond the ends)."""
        x = np.asarray(x, np.float64)
        y, m, h, n = self.log_edf, self.m2, self.h, self.n
        t = (x - self.lt0) / h
        i = np.clip(np.floor(np.nan_to_num(t)).astype(np.int64), 0, n - 2)
        b = t - i
        a = 1.0 - b
        s = a * y[i] + b * y[i + 1] + ((a ** 3 - a) * m[i] + (b ** 3 - b) * m[i + 1]) * (h * h / 6.0)
        d0 = (y[1] - y[0]) / h - h * (2.0 * m[0] + m[1]) / 6.0
        dn = (y[-1] - y[-2]) / h + h * (2.0 * m[-1] + m[-2]) / 6.0
        s = np.where(t >= 0, s, y[0] + d0 * (x - self.lt0))
        return np.where(t > n - 1, y[-1] + dn * (x - (self.lt0 + (n - 1) * h)), s)

    def __call__(self, theta):
        """edf(theta) = exp(S(log theta)); 1 where theta > 1e3 (R/functions.R:1524-1525)."""
        theta = np.asarray(theta, np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.exp(self.log_edf_at(np.log(theta)))
        return np.where(theta > 1e3, 1.0, e)


def load_edf_table(path):
    """The edf table written by ``tools/make_edff_table.py`` (arrays ``lt`` and ``log_edf``)."""
    with np.load(path, allow_pickle=False) as z:
        return EdfTable(z["lt"], z["log_edf"])


# ================================================================== the trend
class Trend:
    """A fitted ``fit_trend`` curve: ``predict(x)``; ``lam`` (the smoothing parameter chosen),
    ``edf`` (the trace of the influence matrix), ``gcv``, ``knots``, ``coef`` (knot values)."""

    def __init__(self, knots, coef, lam, edf, gcv):
        self.knots, self.coef, self.lam, self.edf, self.gcv = knots, coef, lam, edf, gcv

    def predict(self, x):
        x = np.asarray(x, np.float64)
        if self.knots.size < 3:  # a straight line (or a constant)
            return self.coef[0] + (self.coef[1] * x if self.coef.size > 1 else 0.0 * x)
        return _ncs_design(x, self.knots)[0] @ self.coef


def _ncs_design(x, knots):
    """Design matrix of the natural cubic spline over ``knots`` parameterised by its knot
    values (linear beyond the end knots), and its penalty matrix: integral of f''^2 = b' S b."""
    k = knots.size
    h = np.diff(knots)
    D = np.zeros((k - 2, k))
    B = np.zeros((k - 2, k - 2))
    for i in range(k - 2):
        D[i, i], D[i, i + 1], D[i, i + 2] = 1.0 / h[i], -1.0 / h[i] - 1.0 / h[i + 1], 1.0 / h[i + 1]
        B[i, i] = (h[i] + h[i + 1]) / 3.0
        if i + 1 < k - 2:
            B[i, i + 1] = B[i + 1, i] = h[i + 1] / 6.0
    BinvD = np.linalg.solve(B, D)
    F = np.vstack([np.zeros((1, k)), BinvD, np.zeros((1, k))])  # second derivatives at the knots from the values
    S = D.T @ BinvD
    xc = np.clip(x, knots[0], knots[-1])
    j = np.clip(np.searchsorted(knots, xc, side="right") - 1, 0, k - 2)
    hj = h[j]
    am, ap = (knots[j + 1] - xc) / hj, (xc - knots[j]) / hj
    cm, cp = (am ** 3 - am) * hj * hj / 6.0, (ap ** 3 - ap) * hj * hj / 6.0
    n = x.size
    r = np.arange(n)
    X = np.zeros((n, k))
    X[r, j] += am
    X[r, j + 1] += ap
    X += cm[:, None] * F[j] + cp[:, None] * F[j + 1]
    # linear continuation: the end slopes of the spline as functions of the knot values
    s0 = np.zeros(k)
    s0[0], s0[1] = -1.0 / h[0], 1.0 / h[0]
    s0 -= h[0] / 6.0 * F[1]            # f'(knot 0) = (b1 - b0) / h0 - h0 / 6 f''(knot 1)
    s1 = np.zeros(k)
    s1[-2], s1[-1] = -1.0 / h[-1], 1.0 / h[-1]
    s1 += h[-1] / 6.0 * F[-2]
    lo, hi = x < knots[0], x > knots[-1]
    X[lo] += (x[lo] - knots[0])[:, None] * s0[None, :]
    X[hi] += (x[hi] - knots[-1])[:, None] * s1[None, :]
    return X, S


def fit_trend(x, y, weights=None, k=10):
    """A weighted penalised natural cubic regression spline of y on x.

    Knots sit at ``k`` evenly spaced quantiles of x (coincident ones merged), the coefficients
    are the curve's values at the knots, the penalty is the integrated squared second
    derivative, and the smoothing parameter minimises the generalised cross-validation score
    n RSS_w / (n - tr A)^2 over a log-spaced grid followed by a golden-section refinement.
    Beyond the end knots the curve continues as a straight line.  A point of weight 0 has no
    influence.  This is the documented stand-in for ``mgcv::gam(cv2 ~ s(lev, k))``, not mgcv's
    thin-plate fit: the two agree only as far as two reasonable smoothers of the same data do.
    Returns a ``Trend``."""
    x = np.asarray(x, np.float64).ravel()
    y = np.asarray(y, np.float64).ravel()
    w = np.ones_like(x) if weights is None else np.asarray(weights, np.float64).ravel()
    if not (x.shape == y.shape == w.shape):
        raise ValueError("fit_trend: x, y and weights must have the same length")
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(w) & (w > 0)
    x, y, w = x[ok], y[ok], w[ok]
    n = x.size
    if n < 2 or np.ptp(x) == 0:
        if n == 0:
            raise ValueError("fit_trend: no finite point of positive weight")
        return Trend(np.zeros(0), np.array([np.sum(w * y) / np.sum(w)]), np.inf, 1.0, np.nan)
    k = int(k)
    if k < 3:
        raise ValueError("fit_trend: k must be at least 3")
    knots = np.unique(np.quantile(x, np.linspace(0.0, 1.0, k)))
    if knots.size < 3 or n < 4:
        A = np.stack([np.ones(n), x], axis=1)
        coef = np.linalg.lstsq(A * np.sqrt(w)[:, None], y * np.sqrt(w), rcond=None)[0]
        return Trend(knots[:2], coef, np.inf, 2.0, np.nan)
    X, S = _ncs_design(x, knots)
    XtWX = X.T @ (w[:, None] * X)
    XtWy = X.T @ (w * y)
    scale = np.trace(XtWX) / np.trace(S)

    def fit(loglam):
        lam = scale * np.exp(loglam)
        M = XtWX + lam * S
        try:
            sol = np.linalg.solve(M, np.column_stack([XtWy, XtWX]))
        except np.linalg.LinAlgError:
            sol = np.linalg.lstsq(M, np.column_stack([XtWy, XtWX]), rcond=None)[0]
        coef = sol[:, 0]
        tr = float(np.trace(sol[:, 1:]))
        r = y - X @ coef
        rss = float(np.sum(w * r * r))
        den = n - tr
        return (n * rss / (den * den) if den > 0 else np.inf), coef, tr, lam

    grid = np.linspace(np.log(1e-8), np.log(1e8), 65)
    scores = np.array([fit(g)[0] for g in grid])
    b = int(np.argmin(scores))
    lo, hi = grid[max(b - 1, 0)], grid[min(b + 1, grid.size - 1)]
    gr = (np.sqrt(5.0) - 1.0) / 2.0
    c, d = hi - gr * (hi - lo), lo + gr * (hi - lo)
    fc, fd = fit(c)[0], fit(d)[0]
    for _ in range(40):
        if fc <= fd:
            hi, d, fd = d, c, fc
            c = hi - gr * (hi - lo)
            fc = fit(c)[0]
        else:
            lo, c, fc = c, d, fd
            d = lo + gr * (hi - lo)
            fd = fit(d)[0]
    best = min((fit(0.5 * (lo + hi)), fit(grid[b])), key=lambda t: t[0])
    gcv, coef, tr, lam = best
    return Trend(knots, coef, lam, tr, gcv)


# ================================================================== the chi-squared maps
def _holm(p):
    """p.adjust(p, "holm")."""
    p = np.asarray(p, np.float64)
    n = p.size
    o = np.argsort(p, kind="stable")
    adj = np.minimum(1.0, np.maximum.accumulate((n - np.arange(n)) * p[o]))
    out = np.empty(n)
    out[o] = adj
    return out


def _qchisq_upper_log(lq, df, cap):
    """x in [0, cap] with chi2.logsf(x, df) = lq (qchisq(lq, df, lower.tail = FALSE, log.p =
    TRUE) cut at cap): lq = 0 gives 0, lq <= logsf(cap) gives cap; elsewhere a bracketed Newton
    iteration on the log survival function, to 1e-12 relative."""
    from scipy.stats import chi2
    lq = np.asarray(lq, np.float64)
    out = np.full(lq.shape, np.nan)
    nan = np.isnan(lq)
    out[(lq >= 0) & ~nan] = 0.0
    out[(lq <= chi2.logsf(cap, df)) & ~nan] = cap
    todo = np.isnan(out) & ~nan
    if not todo.any():
        return out
    q = lq[todo]
    lo = np.zeros(q.size)
    hi = np.full(q.size, float(cap))
    with np.errstate(all="ignore"):
        x = chi2.isf(np.exp(q), df)
    bad = ~(np.isfinite(x) & (x > lo) & (x < hi))
    x[bad] = 0.5 * (lo[bad] + hi[bad])
    act = np.arange(q.size)          # the entries still iterating
    for _ in range(200):
        xa, qa = x[act], q[act]
        with np.errstate(all="ignore"):
            f = chi2.logsf(xa, df) - qa
            slope = -np.exp(chi2.logpdf(xa, df) - (f + qa))
            up = f > 0                   # logsf falls with x: too large a value means x is too small
            lo[act[up]] = xa[up]
            hi[act[~up]] = xa[~up]
            xn = xa - f / slope
        la, ha = lo[act], hi[act]
        xn = np.where(np.isfinite(xn) & (xn >= la) & (xn <= ha), xn, 0.5 * (la + ha))   # (a zero step ends it)
        x[act] = xn
        done = (np.abs(xn - xa) <= 1e-12 * np.abs(xn)) | (ha - la <= 1e-13 * ha)
        act = act[~done]
        if act.size == 0:
            break
    out[todo] = x
    return out


def adjusted_variance(zval, edf, ncells, max_adj_var=10.0):
    """R/functions.R:1701-1706 for the valid genes: qv = pchisq(zval (edf - 1), edf, upper, log),
    0 where edf <= 1 or |qv| < 1e-10; arv = min(max_adj_var, qchisq(qv, ncells - 1, upper, log)
    / ncells).  scipy has no log-probability quantile: see ``_qchisq_upper_log``."""
    from scipy.stats import chi2
    zval = np.asarray(zval, np.float64)
    edf = np.asarray(edf, np.float64)
    with np.errstate(all="ignore"):
        qv = chi2.logsf(zval * (edf - 1.0), edf)
    qv = np.where(edf <= 1.0, 0.0, qv)
    qv = np.where(np.abs(qv) < 1e-10, 0.0, qv)
    C = int(ncells)
    x = _qchisq_upper_log(qv, C - 1, float(max_adj_var) * C)
    return np.minimum(float(max_adj_var), x / C)


# ================================================================== device stages
def _batch_codes(batch, ncells):
    """pagoda.varnorm's batch handling (1390-1411): levels with fewer than 2 cells join the
    largest; (labels after that or None, int32 codes or None, number of levels or 0)."""
    if batch is None:
        return None, None, 0
    b = np.asarray(batch)
    if b.shape != (ncells,):
        raise ValueError("invalid batch vector supplied: length differs from nrow(models)!")
    levels = sorted(set(b.tolist()))
    per = {lv: int(np.sum(b == lv)) for lv in levels}
    big = max(levels, key=lambda lv: per[lv])
    b = np.array([big if per[v] < 2 else v for v in b.tolist()])
    levels = sorted(set(b.tolist()))
    if len(levels) < 2:
        return b, None, 0
    return b, np.ascontiguousarray([levels.index(v) for v in b.tolist()], np.int32), len(levels)


def _check_edff(edff):
    if not isinstance(edff, EdfTable):
        raise TypeError("edff must be an EdfTable (scde_amd.varnorm.load_edf_table(path))")
    return edff


def _moments_out(out, N, nb):
    r = {"edf": out[0].copy(), "wvar": out[1].copy(), "rowsum_matw": out[2].copy()}
    if nb > 1:
        r.update(bedf=out[3].copy(), bwvar=out[4].copy(), rowsum_bmatw=out[5].copy(), bwvar_ratio=out[6].copy())
    return r


def varnorm_moments(models, counts, edff, avmodes, matw, modes=None, bmatw=None, codes=None, weight_df_power=1.0,
                    theta_range=(1e-2, 1e2), ctx=None):
    """``k_varnorm_moments`` on host inputs (``scde_pagoda_varnorm_moments_host``): counts genes
    x cells, avmodes genes, matw genes x cells; with a batch, modes levels x genes, bmatw and the
    per-cell level codes.  Returns edf, wvar, rowsum_matw (and bedf, bwvar, rowsum_bmatw,
    bwvar_ratio)."""
    edff = _check_edff(edff)
    ctx = ctx or api.default_context()
    cd = np.asfortranarray(np.asarray(counts), dtype=np.int32)
    N, C = cd.shape
    mm, lt, _ = model_matrix(models)
    nb = 0 if codes is None else int(np.max(codes)) + 1
    md = np.ascontiguousarray(np.vstack([np.asarray(avmodes, np.float64)[None, :]] +
                                        ([np.asarray(modes, np.float64)] if nb > 1 else [])))
    w = np.asfortranarray(matw, dtype=np.float64)
    bw = np.asfortranarray(bmatw, dtype=np.float64) if nb > 1 else None
    cc = np.ascontiguousarray(codes, np.int32) if nb > 1 else None
    out = np.zeros((7 if nb > 1 else 3, N))
    check(lib().scde_pagoda_varnorm_moments_host(ctx.handle, _p(cd), N, N, C, _p(mm), lt, _p(md), _p(w), _p(bw),
                                                 _p(cc), nb, _p(edff.table), edff.n, edff.lt0, edff.h,
                                                 float(theta_range[0]), float(theta_range[1]),
                                                 float(weight_df_power), _p(out)))
    return _moments_out(out, N, nb)


def varnorm_matrix(models, counts, matw, arv, codes=None, weight_k=0.9, ctx=None):
    """``k_varnorm_matrix`` on host inputs (``scde_pagoda_varnorm_matrix_host``): matw is the
    weight matrix in use (bmatw with a batch).  Returns (mat, matw), genes x cells."""
    ctx = ctx or api.default_context()
    cd = np.asfortranarray(np.asarray(counts), dtype=np.int32)
    N, C = cd.shape
    mm, _, _ = model_matrix(models)
    nb = 0 if codes is None else int(np.max(codes)) + 1
    w = np.asfortranarray(matw, dtype=np.float64)
    cc = np.ascontiguousarray(codes, np.int32) if nb > 1 else None
    a = np.ascontiguousarray(arv, np.float64)
    mat = np.zeros((N, C), order="F")
    wout = np.zeros((N, C), order="F")
    check(lib().scde_pagoda_varnorm_matrix_host(ctx.handle, _p(cd), N, N, C, _p(mm), _p(w), _p(cc), nb,
                                                float(weight_k), _p(a), _p(mat), _p(wout)))
    return mat, wout


def _trim_counts(models, cd, trim):
    """R/functions.R:1372-1386: Winsorize the magnitudes, map back to counts, drop empty genes.
    The elementwise maps are numpy; the Winsorization is the library's (device) one."""
    from .pagoda import winsorize_matrix
    m = as_model_dict(models)
    a, b = m["corr.a"][None, :], m["corr.b"][None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        fpm = (np.log(cd.astype(np.float64)) - b) / a
        tfpm = np.asarray(winsorize_matrix(fpm, trim))
        back = np.rint(np.exp(tfpm * a + b))   # R's round(): half to even
    back[back < 0] = 0
    back = back.astype(np.int64)
    keep = back.sum(axis=1) > 0
    return np.asfortranarray(back[keep], dtype=np.int32), np.where(keep)[0]


def pagoda_varnorm(models, counts, edff, batch=None, trim=0, prior=None, fit_genes=None,
                   minimize_underdispersion=False, n_cores=1, n_randomizations=100, weight_k=0.9, weight_df_power=1,
                   smooth_df=-1, max_adj_var=10, theta_range=(1e-2, 1e2), gene_length=None, trend=None,
                   return_details=False, ctx=None):
    """pagoda.varnorm (R/functions.R:1347-1811): the variance-normalised expression matrix.

    ``edff``: the ``EdfTable`` of scde's ``scde.edff`` (``load_edf_table``).  ``fit_genes``: gene
    names (with named counts) or row indices the trend is fitted on.  ``trend``: predicted cv2
    (log10 of wvar / avmodes^2) per gene of the (trimmed) matrix, e.g. mgcv's; without it
    ``fit_trend`` is used, which is NOT mgcv's thin-plate fit (see the module text), so results
    agree with R only as far as the two smoothers do.  ``gene_length`` is not built.

    Returns the ``varinfo`` dict the PAGODA functions take: mat, matw (genes x cells), arv, modes
    (levels x genes with a batch, else avmodes), avmodes, prior, edf, batch, trim, genes; with a
    batch bwvar_ratio; with a trim that dropped rows ``kept`` (their indices in the input).
    ``return_details`` adds wvar, vi, zval and trend (the predicted cv2 of every gene)."""
    from .prior import expression_prior
    if gene_length is not None:
        raise NotImplementedError("pagoda_varnorm: gene_length (the second smooth of the trend) is not built")
    edff = _check_edff(edff)
    ctx = ctx or api.default_context()
    cd, genes = api._align_counts(models, counts)
    kept = None
    if trim > 0:
        cd, kept = _trim_counts(models, cd, trim)
        if genes is not None:
            genes = [genes[i] for i in kept]
    N, C = cd.shape
    mm, lt, sq = model_matrix(models)
    if mm.shape[0] != C:
        raise ValueError("counts and models disagree on the number of cells")
    blabels, codes, nb = _batch_codes(batch, C)
    if prior is None:
        prior = expression_prior(models, cd, length_out=400, show_plot=False, ctx=ctx)
    px = np.ascontiguousarray(prior["x"], np.float64)
    nm = 1 + nb if nb > 1 else 1
    modes = np.zeros((nm, N))
    dc = api.DeviceCounts(ctx, cd)
    L = lib()
    try:
        # stage 1: weights (kept in HBM by the context; only the modes come back)
        check(L.scde_pagoda_varnorm_weights_dev(ctx.handle, dc.ptr, N, N, C, _p(mm), lt, sq, _p(px), len(px),
                                                int(n_randomizations), int(n_cores), _p(codes), nb, 1, _p(modes),
                                                None, None))
        # stage 2: moments
        out = np.zeros((7 if nb > 1 else 3, N))
        check(L.scde_pagoda_varnorm_moments_dev(ctx.handle, dc.ptr, N, N, C, _p(mm), lt, None, None, None, _p(codes),
                                                nb, _p(edff.table), edff.n, edff.lt0, edff.h, float(theta_range[0]),
                                                float(theta_range[1]), float(weight_df_power), _p(out)))
        mom = _moments_out(out, N, nb)
        # stage 3: host statistics
        fit_mask = None
        if fit_genes is not None:
            fit_mask = np.zeros(N, bool)
            fg = list(fit_genes)
            if genes is not None and fg and isinstance(fg[0], str):
                s = set(fg)
                fit_mask[[i for i, g in enumerate(genes) if g in s]] = True
            else:
                idx = np.asarray(fg, np.int64)
                if kept is not None:  # indices refer to the input rows
                    pos = {int(r): i for i, r in enumerate(kept)}
                    idx = np.array([pos[int(r)] for r in idx if int(r) in pos], np.int64)
                fit_mask[idx] = True
        st = varnorm_statistics(modes[0], mom, C, fit_mask=fit_mask, trend=trend, smooth_df=smooth_df,
                                minimize_underdispersion=minimize_underdispersion, max_adj_var=max_adj_var)
        # stage 4: the matrix
        mat = np.zeros((N, C), order="F")
        wout = np.zeros((N, C), order="F")
        arv = np.ascontiguousarray(st["arv"])
        check(L.scde_pagoda_varnorm_matrix_dev(ctx.handle, dc.ptr, N, N, C, _p(mm), None, _p(codes), nb,
                                               float(weight_k), _p(arv), _p(mat), _p(wout)))
    finally:
        dc.free()
    res = {"mat": mat, "matw": wout, "arv": st["arv"], "modes": modes[1:].copy() if nb > 1 else modes[0].copy(),
           "avmodes": modes[0].copy(), "prior": prior, "edf": mom["edf"], "batch": blabels,
           "trim": trim, "genes": genes}
    if nb > 1:
        res["bwvar_ratio"] = mom["bwvar_ratio"]
    if kept is not None:
        res["kept"] = kept
    if return_details:
        res.update(wvar=st["wvar"], vi=st["vi"], zval=st["zval"], trend=st["trend"])
    return res


def varnorm_statistics(avmodes, moments, ncells, fit_mask=None, trend=None, smooth_df=-1,
                       minimize_underdispersion=False, max_adj_var=10):
    """The host part of pagoda.varnorm between its two kernels (R/functions.R:1610-1706), on
    N-vectors: ``moments`` is what ``k_varnorm_moments`` returned.  Returns arv (NaN outside vi),
    vi, wvar (the batch one with a batch), zval (NaN outside vi) and trend (predicted cv2)."""
    from scipy.stats import chi2
    avmodes = np.asarray(avmodes, np.float64)
    N = avmodes.size
    batched = "bwvar" in moments
    wvar = moments["bwvar"] if batched else moments["wvar"]
    rsw = moments["rowsum_bmatw"] if batched else moments["rowsum_matw"]
    edf = moments["edf"]
    vi = (rsw > 0) & np.isfinite(wvar) & (wvar > 0)
    fvi = vi & fit_mask if fit_mask is not None else vi.copy()
    if not fvi.any():
        raise ScdeError("unable to find a set of valid genes to establish the variance fit")
    with np.errstate(divide="ignore", invalid="ignore"):
        lev = np.log10(avmodes)
        cv2 = np.log10(wvar / avmodes ** 2)
    if trend is not None:
        pred = np.asarray(trend, np.float64)
        if pred.shape != (N,):
            raise ValueError(f"trend must hold one predicted cv2 per gene ({N}), got shape {pred.shape}")
        pred = pred.copy()
    else:
        k = int(smooth_df) if smooth_df > 0 else 10
        tr = fit_trend(lev[fvi], cv2[fvi], weights=rsw[fvi], k=k)
        with np.errstate(invalid="ignore"):
            pred = tr.predict(lev)
        if minimize_underdispersion:  # 1654-1664
            z0 = 10.0 ** (cv2[fvi] - pred[fvi])
            pv = chi2.cdf(z0 * (edf[fvi] - 1.0), edf[fvi])
            pv[edf[fvi] <= 1.0] = 0.0
            pv = _holm(pv)
            with np.errstate(divide="ignore"):
                wt = (np.minimum(10.0, -np.log(pv)) + 1.0) * rsw[fvi]
            tr = fit_trend(lev[fvi], cv2[fvi], weights=wt, k=k)
            with np.errstate(invalid="ignore"):
                pred = tr.predict(lev)
    zval = np.full(N, np.nan)
    with np.errstate(over="ignore", invalid="ignore"):
        zval[vi] = 10.0 ** (cv2[vi] - pred[vi])
        if batched:
            r = moments["bwvar_ratio"][vi]
            zval[vi] = zval[vi] * np.minimum(r, 1.0 / r)
    arv = np.full(N, np.nan)
    arv[vi] = adjusted_variance(zval[vi], edf[vi], ncells, max_adj_var)
    return {"arv": arv, "vi": vi, "wvar": wvar, "zval": zval, "trend": pred}


# ================================================================== pagoda.subtract.aspect
def pagoda_subtract_aspect(varinfo, aspect, center=True, ctx=None):
    """pagoda.subtract.aspect (R/functions.R:1850-1862), on the device: the weighted projection
    of every gene on the cell pattern ``aspect`` is removed from ``varinfo["mat"]`` and the rows
    are re-centred (``center``).  Returns a copy of ``varinfo`` with the new ``mat``."""
    mat = np.asfortranarray(varinfo["mat"], dtype=np.float64)
    matw = np.asfortranarray(varinfo["matw"], dtype=np.float64)
    v = np.ascontiguousarray(aspect, np.float64).ravel()
    if mat.ndim != 2 or matw.shape != mat.shape:
        raise ValueError("varinfo mat and matw must be genes x cells matrices of the same shape")
    if v.size != mat.shape[1]:
        raise ValueError("aspect should be a numeric vector of the same length as the number of cells "
                         "(i.e. ncol(varinfo$mat))")
    ctx = ctx or api.default_context()
    out = np.zeros(mat.shape, order="F")
    check(lib().scde_pagoda_subtract_aspect_host(ctx.handle, _p(mat), _p(matw), mat.shape[0], mat.shape[1], _p(v),
                                                 int(bool(center)), _p(out)))
    res = dict(varinfo)
    res["mat"] = out
    return res
