"""``pagoda.top.aspects`` (R/functions.R:2277-2456) with ``pagoda.effective.cells`` (2000-2014)
and the helpers ``gev.t``, ``pgev.upper.log`` and ``bh.adjust`` (5096-5124): the overdispersion
score of every gene set and gene cluster, and the aspect matrix ``tam`` that
``pagoda_reduce_loading_redundancy`` takes.

Almost all of it is host statistics on vectors with one entry per set and component
(``top_aspects_table``); the Tracy-Widom law comes from ``scde_amd.rmt``.  The one pass over
(valid aspects x cells) -- centring and scaling the scores, normalising their weights -- runs on
the GPU (csrc/top_aspects.hip; contract in include/scde_hip.h).  ``return_table`` and
``return_genes`` touch no GPU.

``pwpca`` is what ``pagoda_pathway_wPCA`` returns ({set name: {"xp", "z", "sd", "n"}}; ``None``
entries are skipped throughout), ``clpca`` what ``pagoda_gene_clusters`` returns.  ``plot`` and
the commented-out ``vshift`` / ``ev`` path (both are 0 in R) are not restated.

Deviations from R, each in the docstring of its function and in DESIGN.md section 4.13: the
Tracy-Widom tail is the law's own everywhere (``tw_tail_from``); ``pagoda_effective_cells``
states its own minimiser; a NaN score counts as not valid.  Nothing here was checked against R,
RMTstat or extRemes.
"""
from __future__ import annotations

import math

import numpy as np

from . import rmt

Z_SCORE = 1.959963984540054   # qnorm(0.05 / 2, lower.tail = FALSE)


# ================================================================== log-space helpers
def _bracketed_newton(f, lo, hi, x, rel=1e-13):
    """Per entry the root in [lo, hi] of a decreasing function: f(x, active) returns (value,
    slope) of the entries ``active``.  Newton steps kept inside the bracket, bisection when a
    step leaves it or is not finite."""
    act = np.arange(x.size)
    for _ in range(300):
        xa = x[act]
        with np.errstate(all="ignore"):
            v, slope = f(xa, act)
            up = v > 0                       # decreasing: a positive value means x is too small
            lo[act[up]] = xa[up]
            hi[act[~up]] = xa[~up]
            xn = xa - v / slope
        la, ha = lo[act], hi[act]
        xn = np.where(np.isfinite(xn) & (xn >= la) & (xn <= ha), xn, 0.5 * (la + ha))
        x[act] = xn
        done = (np.abs(xn - xa) <= rel * np.abs(xn)) | (ha - la <= rel * np.maximum(np.abs(la), np.abs(ha)))
        act = act[~done]
        if act.size == 0:
            break
    return x


def qnorm_upper_log(lp):
    """``qnorm(lp, lower.tail = FALSE, log.p = TRUE)``: the z with log(1 - Phi(z)) = lp, by a
    bracketed Newton iteration on ``scipy.special.log_ndtr(-z)``.  exp(lp) is never formed, so
    log probabilities below -745 (z above 38.5) are resolved.  lp = 0 gives -inf, -inf gives
    +inf; NaN and lp > 0 give NaN (R warns and gives NaN).  An upper tail within 1e-300 of 1
    (lp > -1e-300) gives -inf."""
    from scipy.special import log_ndtr
    lp = np.asarray(lp, dtype=np.float64)
    out = np.full(lp.shape, np.nan)
    with np.errstate(invalid="ignore"):
        out[lp == -np.inf] = np.inf
        out[(lp <= 0) & (lp > -1e-300)] = -np.inf
        todo = (lp <= -1e-300) & (lp > -np.inf)
    if todo.any():
        q = lp[todo]
        lo = np.full(q.size, -40.0)
        hi = np.sqrt(-2.0 * q) + 2.0         # log(1 - Phi(z)) <= -z^2 / 2 for z >= 0
        x0 = np.where(q < -2.0, np.sqrt(np.maximum(-2.0 * q - np.log(np.maximum(-4.0 * math.pi * q, 1.0)), 0.0)), 0.0)

        def f(z, act):
            ls = log_ndtr(-z)
            return ls - q[act], -np.exp(-0.5 * z * z - 0.5 * math.log(2.0 * math.pi) - ls)
        out[todo] = _bracketed_newton(f, lo, hi, x0)
    return out if out.ndim else float(out)


def bh_adjust_log(lp):
    """``bh.adjust(lp, log = TRUE)`` (R/functions.R:5111-5124): Benjamini-Hochberg on log
    p-values, sorted increasing (ties in order), ``lp + log(N / rank)``, the running minimum
    from the largest down.  NaN entries are skipped (N counts the others) and stay NaN.  As in
    R the result is not capped at log 1."""
    lp = np.asarray(lp, dtype=np.float64)
    out = lp.copy()
    ok = np.nonzero(~np.isnan(lp.ravel()))[0]
    x = lp.ravel()[ok]
    if x.size:
        o = np.argsort(x, kind="stable")
        q = x[o] + np.log(x.size / np.arange(1.0, x.size + 1.0))
        a = np.minimum.accumulate(q[::-1])[::-1]
        res = np.empty(x.size)
        res[o] = a
        out.reshape(-1)[ok] = res
    return out


def pgev_upper_log(x, loc, scale, shape=0.0):
    """``pgev.upper.log`` (R/functions.R:5104-5108): the log upper tail of a generalised
    extreme value law.  t = ``gev.t(log = TRUE)`` = min(0, -(x - loc) / scale) for shape 0, else
    min(0, -log(max(0, 1 + shape (x - loc) / scale)) / shape); for -5 < t < 0 the result is
    log(-expm1(-exp(t))), elsewhere t itself (below -5 the two differ by less than exp(-5) / 2)."""
    x = np.asarray(x, dtype=np.float64)
    y = (x - loc) / scale
    with np.errstate(all="ignore"):
        t = -y if shape == 0 else (-1.0 / shape) * np.log(np.maximum(0.0, 1.0 + shape * y))
        t = np.array(np.minimum(0.0, t), dtype=np.float64)
        sw = (t > -5.0) & (t < 0.0)
        t[sw] = np.log(-np.expm1(-np.exp(t[sw])))
    return t if t.ndim else float(t)


def qgumbel_upper(p, loc, scale):
    """``extRemes::qevd(p, loc, scale, shape = 0, lower.tail = FALSE)``: loc - scale log(-log1p(-p))."""
    return loc - scale * math.log(-math.log1p(-p))


def qchisq_upper_log(lp, df):
    """``qchisq(lp, df, lower.tail = FALSE, log.p = TRUE)``.  Down to lp = -600 this is
    ``varnorm._qchisq_upper_log``; below, where scipy's chi2.logsf has underflowed, the same
    bracketed Newton iteration on log Q(df / 2, x / 2) from Legendre's continued fraction.
    lp = -inf gives inf."""
    from scipy.special import gammaln

    from .varnorm import _qchisq_upper_log
    lp = np.asarray(lp, dtype=np.float64)
    out = np.full(lp.shape, np.nan)
    out[lp == -np.inf] = np.inf
    with np.errstate(invalid="ignore"):
        near = (lp >= -600.0)
        deep = (lp < -600.0) & (lp > -np.inf)
    if near.any():
        # a cap above every root: log Q <= -(df / 2) (t - 1 - log t) at x = df t, and t - 1 - log t >= t / 3 from 4 on
        out[near] = _qchisq_upper_log(lp[near], df, max(4.0 * df, 6.0 * 600.0))
    if deep.any():
        q = lp[deep]
        a = 0.5 * df
        lo = np.full(q.size, 2.0 * (a + 1.0))
        hi = np.maximum(4.0 * df, -6.0 * q)
        x0 = np.minimum(hi, np.maximum(lo, -2.0 * q))

        def f(x, act):
            ls = rmt._log_upper_gamma(a, 0.5 * x) - gammaln(a)
            return ls - q[act], -0.5 * np.exp((a - 1.0) * np.log(0.5 * x) - 0.5 * x - gammaln(a) - ls)
        out[deep] = _bracketed_newton(f, lo, hi, x0)
    return out if out.ndim else float(out)


# ================================================================== pagoda.effective.cells
def _sets(pwpca):
    """[(name, entry)] of the entries that are not None, in order."""
    return [(str(k), v) for k, v in pwpca.items() if v is not None]


def _n_cells_of(sets):
    if not sets:
        raise ValueError("pwpca holds no gene set")
    return int(np.asarray(sets[0][1]["xp"]["scores"]).shape[0])


def _effective_cells_terms(sn, v, sp):
    """(objective, its derivative) of R/functions.R:2006-2011 at sn."""
    k = -rmt.TW1_MEAN
    d = sn * sn + 0.5
    c = np.cbrt(1.0 / sn + 1.0 / sp)
    a = (sn + sp) ** 2
    b = (sn + sp) * c
    fit = (a - k * b) / d
    da = 2.0 * (sn + sp)
    db = c + (sn + sp) * (-1.0 / (3.0 * sn * sn)) / (c * c)
    dfit = ((da - k * db) * d - (a - k * b) * 2.0 * sn) / (d * d)
    r = v - fit
    return float(np.sum(r * r)), float(-2.0 * np.sum(r * dfit))


def pagoda_effective_cells(pwpca, start=None):
    """``pagoda.effective.cells`` (R/functions.R:2000-2014): the effective number of cells
    ``sn^2 + 1/2``, where sn in [1, n_cells] minimises

        sum((v - vfit(sn, sp))^2),
        vfit = (sn + sp)^2 / (sn^2 + 1/2) - 1.2065335745820 (sn + sp) (1/sn + 1/sp)^(1/3) / (sn^2 + 1/2)

    over the random sets' PC1 variances v = z[:, 0]^2 of every gene set (``None`` entries
    skipped), sp = sqrt(n - 1/2) with n the set's size.  The bound is on sn, not on sn^2, as
    in R, so the result can reach n_cells^2 + 1/2.

    The minimiser is stated here, not R's: from x0 = min(start or 10 n_cells, n_cells), if x0
    is the upper bound and the objective does not decrease to its left, the bound is returned;
    otherwise the first local minimum met on the way down from x0 (steps doubling until the
    objective rises, then Brent's bounded minimiser on the bracket, then the root of the
    analytic derivative beside it), located to 1e-10 relative; a descent that reaches a bound
    returns that bound.  R's ``nlminb`` (PORT) from the same start agrees with this only to its
    own tolerance and only when it stops in the same basin; that was not checked."""
    from scipy.optimize import brentq, minimize_scalar
    sets = _sets(pwpca)
    n_cells = _n_cells_of(sets)
    v, sp = [], []
    for _, x in sets:
        z = np.asarray(x["z"], dtype=np.float64)
        z = z.reshape(z.shape[0], -1) if z.size else np.zeros((0, 1))
        v.append(z[:, 0] ** 2)
        sp.append(np.full(z.shape[0], math.sqrt(x["n"] - 0.5)))
    v, sp = np.concatenate(v), np.concatenate(sp)
    if v.size == 0:
        raise ValueError("pagoda_effective_cells: pwpca holds no randomised sets (z is empty)")
    if not np.all(np.isfinite(v)):
        raise ValueError("pagoda_effective_cells: a randomised variance is not finite")
    lb, ub = 1.0, float(n_cells)
    if ub <= lb:
        return ub * ub + 0.5
    of = lambda s: _effective_cells_terms(s, v, sp)[0]   # noqa: E731
    x0 = min(float(start) if start is not None else 10.0 * n_cells, ub)
    x0 = max(x0, lb)
    f0 = of(x0)
    h = 1e-4 * x0
    left, right = max(lb, x0 - h), min(ub, x0 + h)
    fl = of(left) if left < x0 else math.inf
    fr = of(right) if right > x0 else math.inf
    if fl >= f0 and fr >= f0:
        if x0 in (lb, ub):
            return x0 * x0 + 0.5           # the bound: nothing lower beside it
        a, c = left, right                 # x0 sits in a minimum's bracket already
    else:
        sgn = -1.0 if fl < fr else 1.0
        a, b, fb = x0, (left if sgn < 0 else right), min(fl, fr)
        while True:
            h *= 2.0
            nxt = min(ub, max(lb, b + sgn * h))
            if nxt == b:                   # still falling at a bound
                return b * b + 0.5
            fn = of(nxt)
            if fn >= fb:
                a, c = (nxt, a) if sgn < 0 else (a, nxt)
                break
            a, b, fb = b, nxt, fn
    res = minimize_scalar(of, bounds=(a, c), method="bounded", options={"xatol": 1e-10 * a, "maxiter": 500})
    x = float(res.x)
    # the objective is flat to second order at its minimum; its derivative is not
    g = lambda s: _effective_cells_terms(s, v, sp)[1]    # noqa: E731
    d = 1e-5 * x
    lo_, hi_ = max(a, x - d), min(c, x + d)
    if g(lo_) < 0.0 < g(hi_):
        x = float(brentq(g, lo_, hi_, xtol=1e-13 * x, rtol=1e-12))
    return x * x + 0.5


# ================================================================== the table
def _set_rows(sets, first):
    """R/functions.R:2285-2290 / 2331-2338: per set and component i (1-based, from ``first``),
    var = sd^2, n, npc, shz (NaN without xp["randvar"]; else (var - mean) / sd, sd with the
    n - 1 denominator)."""
    cols = {k: [] for k in ("i", "var", "n", "npc", "shz")}
    for j, (name, x) in enumerate(sets):
        var = np.asarray(x["sd"], dtype=np.float64).ravel() ** 2
        k = np.asarray(x["xp"]["scores"]).reshape(len(x["xp"]["scores"]), -1).shape[1]
        if var.size != k:
            raise ValueError(f"{name!r}: sd has {var.size} entries for {k} component(s)")
        rv = x["xp"].get("randvar")
        if rv is None:
            shz = np.full(k, np.nan)
        else:
            rv = np.asarray(rv, dtype=np.float64).ravel()
            with np.errstate(all="ignore"):
                shz = (var - rv.mean()) / (rv.std(ddof=1) if rv.size > 1 else np.nan)
        cols["i"].append(np.full(k, first + j, dtype=np.int64))
        cols["var"].append(var)
        cols["n"].append(np.full(k, float(x["n"])))
        cols["npc"].append(np.arange(1, k + 1, dtype=np.int64))
        cols["shz"].append(shz)
    return {k: np.concatenate(v) for k, v in cols.items()}


def _z_adjust(z):
    """qnorm(bh.adjust(pnorm(z, lower.tail = FALSE, log.p = TRUE), log = TRUE), lower.tail = FALSE, log.p = TRUE)"""
    from scipy.special import log_ndtr
    return qnorm_upper_log(bh_adjust_log(log_ndtr(-np.asarray(z, dtype=np.float64))))


def top_aspects_table(pwpca, clpca=None, n_cells=None, z_score=Z_SCORE, adjust_scores=True, score_alpha=0.05,
                      effective_cells_start=None, tw_tail_from=None):
    """R/functions.R:2280-2416, host only: the table behind ``pagoda_top_aspects`` as a dict of
    equal-length arrays, one entry per gene set (in ``pwpca`` order, ``None`` skipped) and
    component, then -- with ``clpca`` -- per gene cluster of ``clpca["cl.goc"]`` and component.

      i, npc         the set (1-based among the sets kept; clusters follow, shifted by their
                     number) and the component (1-based); name: the set's name
      var, n         sd^2 and the set's size
      shz            (var - mean(randvar)) / sd(randvar), NaN without xp["randvar"]
      exp            gene sets: ``rmt.q_wishart_max_upper(0.5, n_cells, n)``; clusters:
                     location sqrt(pv) + pvar
      z              gene sets: ``qnorm_upper_log(rmt.p_wishart_max_upper_log(var, n_cells, n,
                     tw_tail_from))``; clusters: ``qnorm_upper_log(pgev_upper_log(varst, location,
                     scale))`` with pm, pv as in ``rmt.score_varm``, pvar = the prediction of
                     clpca["clvlm"] (coefficients pm, n), varst = (var - pvar) / sqrt(pv) and
                     (location, scale) = ``rmt.gumbel_fit(clpca["varm"]["varst"])``, shape 0
      cz             z Benjamini-Hochberg adjusted in log space, the gene sets and the clusters
                     each among themselves
      ub, ub_stringent   the upper quantile at score_alpha / 2 and at score_alpha / rows / 2
                     (rows: of the gene sets, or of the clusters) of the same two null models
      adj_shz        shz adjusted over all rows (NaN skipped)
      score, oec     var / exp and var / ub
      valid          (cz if adjust_scores else z) >= z_score

    and "n_cells" (given, or ``pagoda_effective_cells(pwpca, effective_cells_start)``) and
    "sets", the [(name, entry)] that ``i`` - 1 indexes.  A NaN z counts as not valid (R's
    comparison gives NA there and ``vdf[NA, ]`` an NA row).  The Tracy-Widom tail is the law's own;
    ``tw_tail_from`` switches to R's gamma formula from that value of the scaled statistic on
    (``rmt.p_wishart_max_upper_log``).  When no row is valid: ValueError with R's message."""
    sets = _sets(pwpca)
    _n_cells_of(sets)
    if n_cells is None:
        n_cells = pagoda_effective_cells(pwpca, start=effective_cells_start)
    n_cells = float(n_cells)
    t = _set_rows(sets, 1)
    nrows = len(t["var"])
    par = rmt.wishart_max_par(n_cells, t["n"])
    q = {p: rmt.qtw_upper(p) for p in (0.5, score_alpha / 2, score_alpha / nrows / 2)}
    t["exp"] = par["centering"] + par["scaling"] * q[0.5]
    t["z"] = qnorm_upper_log(rmt.p_wishart_max_upper_log(t["var"], n_cells, t["n"], tail_from=tw_tail_from))
    t["cz"] = _z_adjust(t["z"])
    t["ub"] = par["centering"] + par["scaling"] * q[score_alpha / 2]
    t["ub_stringent"] = par["centering"] + par["scaling"] * q[score_alpha / nrows / 2]
    if clpca is not None:
        csets = _sets(clpca["cl.goc"])
        c = _set_rows(csets, len(sets) + 1)
        xf = rmt.gumbel_fit(np.asarray(clpca["varm"]["varst"], dtype=np.float64))
        loc, scale = xf["location"], xf["scale"]
        par = rmt.wishart_max_par(n_cells, c["n"])
        pm = par["centering"] + rmt.TW1_MEAN * par["scaling"]
        pv = rmt.TW1_VAR * par["scaling"]
        coef = clpca["clvlm"]["coefficients"]
        pvar = float(coef["pm"]) * pm + float(coef["n"]) * c["n"]
        varst = (c["var"] - pvar) / np.sqrt(pv)
        c["exp"] = loc * np.sqrt(pv) + pvar
        c["z"] = qnorm_upper_log(pgev_upper_log(varst, loc, scale))
        c["cz"] = _z_adjust(c["z"])
        c["ub"] = qgumbel_upper(score_alpha / 2, loc, scale) * np.sqrt(pv) + pvar
        c["ub_stringent"] = qgumbel_upper(score_alpha / 2 / len(varst), loc, scale) * np.sqrt(pv) + pvar
        t = {k: np.concatenate([t[k], c[k]]) for k in t}
        sets = sets + csets
    t["adj_shz"] = _z_adjust(t["shz"])
    with np.errstate(all="ignore"):
        t["score"] = t["var"] / t["exp"]
        t["oec"] = t["var"] / t["ub"]
        t["valid"] = (t["cz"] if adjust_scores else t["z"]) >= z_score   # (NaN compares false)
    t["name"] = [sets[i - 1][0] for i in t["i"]]
    t["n_cells"] = n_cells
    t["sets"] = sets
    if not t["valid"].any():
        raise ValueError(f"no significantly overdispersed pathways found at z.score threshold of {z_score:.15g}")
    return t


def _df(t, rows):
    import pandas as pd
    return pd.DataFrame({"name": [t["name"][r] for r in rows], "npc": t["npc"][rows], "n": t["n"][rows].astype(np.int64),
                         "score": t["score"][rows], "z": t["z"][rows], "adj.z": t["cz"][rows], "sh.z": t["shz"][rows],
                         "adj.sh.z": t["adj_shz"][rows]})


def _rotation_column(name, x, npc):
    rot = np.asarray(x["xp"]["rotation"], dtype=np.float64)
    if rot.ndim == 1:
        rot = rot[:, None]
    genes = x["xp"]["rotation_names"]
    if len(genes) != rot.shape[0]:
        raise ValueError(f"{name!r}: rotation and rotation_names differ in length")
    return genes, np.abs(rot[:, npc - 1])


def _gene_weights(t, rows):
    """R/functions.R:2426-2428: per valid row the |loadings| of at least a third of the row's
    largest; per gene the maximum over the rows; keys sorted."""
    gw = {}
    for r in rows:
        name, x = t["sets"][t["i"][r] - 1]
        genes, s = _rotation_column(name, x, int(t["npc"][r]))
        keep = s >= s.max() / 3.0
        for g, val in zip(np.asarray(genes, dtype=object)[keep], s[keep]):
            g = str(g)
            if val > gw.get(g, -1.0):
                gw[g] = float(val)
    return {g: gw[g] for g in sorted(gw)}


def _scale_rows_dev(x, w, num, ctx):
    """The device stage: (xv, xvw) of m x C row-major host arrays (scde_top_aspects)."""
    from . import api
    from ._lib import check, lib
    ctx = ctx or api.default_context()
    m, c = x.shape
    xv, xvw = np.empty((m, c)), np.empty((m, c))
    check(lib().scde_top_aspects(ctx.handle, api._p(x), api._p(w), api._p(num), m, c, api._p(xv), api._p(xvw)))
    return xv, xvw


def pagoda_top_aspects(pwpca, clpca=None, n_cells=None, z_score=Z_SCORE, return_table=False, return_genes=False,
                       adjust_scores=True, score_alpha=0.05, use_oe_scale=False, effective_cells_start=None,
                       tw_tail_from=None, ctx=None):
    """``pagoda.top.aspects`` (R/functions.R:2277-2456; no ``plot``): the significantly
    overdispersed aspects of ``pwpca`` (and of the gene clusters ``clpca``), from
    ``top_aspects_table`` (which documents the columns, ``n_cells``, ``tw_tail_from`` and the
    treatment of NaN).

      return_table   a DataFrame of the valid rows -- name, npc, n, score, z, adj.z, sh.z,
                     adj.sh.z -- by decreasing score, ties in table order.  No GPU is touched.
      return_genes   {gene: weight}, keys sorted: per valid row the |loadings| of its component
                     that reach a third of the row's largest, per gene the maximum over the
                     rows.  No GPU is touched.
      otherwise      {"xv", "xvw", "names", "gw", "df"}, a ``tam`` as ``scde_amd.aspects`` takes
                     it: per valid row, in table order, names = "#PC<npc># <set>";
                     xv = (scores - mean) * num / sqrt(var(scores)) with var's denominator
                     cells - 1 and num = sqrt(qchisq(pnorm(z, upper, log), n_cells, upper, log) /
                     n_cells), or the row's score with ``use_oe_scale``; xvw = scoreweights /
                     their sum; gw as above; df the DataFrame of all rows in table order.
                     Only the valid rows of the scores and weights are gathered (m x cells),
                     and one launch of csrc/top_aspects.hip does the rest; a constant score row
                     comes out NaN, as R's arithmetic gives it.

    No valid row raises ValueError with R's message."""
    t = top_aspects_table(pwpca, clpca, n_cells=n_cells, z_score=z_score, adjust_scores=adjust_scores,
                          score_alpha=score_alpha, effective_cells_start=effective_cells_start,
                          tw_tail_from=tw_tail_from)
    rows = np.nonzero(t["valid"])[0]
    if return_table:
        o = np.argsort(-t["score"][rows], kind="stable")
        return _df(t, rows[o]).reset_index(drop=True)
    gw = _gene_weights(t, rows)
    if return_genes:
        return gw
    from scipy.special import log_ndtr
    cells = _n_cells_of(t["sets"])
    x = np.empty((len(rows), cells))
    w = np.empty((len(rows), cells))
    for k, r in enumerate(rows):
        name, e = t["sets"][t["i"][r] - 1]
        sc = np.asarray(e["xp"]["scores"], dtype=np.float64)
        sw = np.asarray(e["xp"]["scoreweights"], dtype=np.float64)
        sc, sw = sc.reshape(sc.shape[0], -1), sw.reshape(sw.shape[0], -1)
        if sc.shape[0] != cells or sw.shape != sc.shape:
            raise ValueError(f"{name!r}: scores and scoreweights must be {cells} cells x components")
        x[k] = sc[:, t["npc"][r] - 1]
        w[k] = sw[:, t["npc"][r] - 1]
    if use_oe_scale:
        num = np.ascontiguousarray(t["score"][rows])
    else:
        with np.errstate(all="ignore"):
            num = np.sqrt(qchisq_upper_log(log_ndtr(-t["z"][rows]), t["n_cells"]) / t["n_cells"])
    xv, xvw = _scale_rows_dev(x, w, np.ascontiguousarray(num, dtype=np.float64), ctx)
    names = [f"#PC{int(t['npc'][r])}# {t['name'][r]}" for r in rows]
    return {"xv": xv, "xvw": xvw, "names": names, "gw": gw, "df": _df(t, np.arange(len(t["var"])))}


__all__ = ["Z_SCORE", "bh_adjust_log", "pagoda_effective_cells", "pagoda_top_aspects", "pgev_upper_log",
           "qchisq_upper_log", "qgumbel_upper", "qnorm_upper_log", "top_aspects_table"]
