"""Host statistics of ``pagoda.gene.clusters``' null model (R/functions.R:2196-2211), plain numpy:
the Tracy-Widom centring and scaling of a white Wishart matrix's largest eigenvalue, the
regression of the sampled PC1 variances on it, and the Gumbel fit of the standardised residuals.

Neither RMTstat nor extRemes was run against this module; what each function restates, and how far
that was checked, is in its docstring and in DESIGN.md section 4.8.
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
