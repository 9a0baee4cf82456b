"""One posterior-table column in 60-digit arithmetic (mpmath): the arbiter where the float64
oracle's own rounding matters (theta outside the fitted range, tests/test_table_edges.py and
tests/test_gpu_table_edges.py group W).

What oracle/scde_oracle.c o_cell_tables computes per (cell, count x), restated from its
mathematical definition (include/scde_hip.h layer 1; constant theta, plain logit concomitant):

    mu_k   = exp(mag_k corr.a + corr.b), and mu_k = x at the one point the count overrides
    p_k    = theta / (theta + mu_k), q_k = 1 - p_k
    nb_k   = log dnbinom(x; theta, p_k) = lgamma(x + theta) - lgamma(theta) - lgamma(x + 1)
             + theta log p_k + x log q_k
    cfp_k  = 1 / (exp(mag_k conc.a + conc.b) + 1)
    fp     = log dpois(x; exp(fail.r))
    e_k    = exp(nb_k + log(1 - cfp_k)) + exp(log cfp_k + fp)
    T_k    = max(log(e_k / sum_j e_j), minlogprob)

The float64 model parameters, magnitudes and the count are taken as exact, and so is every
intermediate (p_k included): forms that would cancel at 60 digits are written without the
cancellation (lgamma(x + theta) - lgamma(theta) as a sum of x logs; log p_k as -log1p(mu_k /
theta)), which changes nothing mathematically.  The DISCRETE choices are the float64 oracle's and
are shared with it, as ref_keep is in tests/test_distance.py: the override point (x > mu_k and
x < mu_k+1 on the float64 mu, libm's exp) and, through `clamped`, the points the oracle clamps
at minlogprob.  Domain: finite parameters and magnitudes, theta > 0, exp(fail.r) > 0.
"""
import math

import mpmath as mp
import numpy as np

DPS = 60


def override_point(corr_a, corr_b, mag, x):
    """The grid point whose mu the count replaces (src/jpmatLogBoot.cpp:170-172), on float64 mu."""
    G = len(mag)
    mu = [math.exp(float(m) * corr_a + corr_b) for m in mag]
    out = [k for k in range(G) if (k < G - 1 and x > mu[k] and x < mu[k + 1]) or (k == G - 1 and x > mu[k])]
    return out  # (every such point: more than one where mu is not monotone)


def column(model_row, mag, x, minlogprob, clamped=None):
    """T_k, k < len(mag), as mpf values.  model_row: conc.b, conc.a, fail.r, corr.b, corr.a,
    corr.theta (float64); x: the count; clamped: boolean per point, the oracle's clamp decisions
    (None: decided here, T_k < minlogprob)."""
    with mp.workdps(DPS):
        concb, conca, failr, corrb, corra, theta = (mp.mpf(float(v)) for v in model_row[:6])
        x = int(x)
        G = len(mag)
        over = set(override_point(float(model_row[4]), float(model_row[3]), mag, x))
        # the (x, theta)-only part of log dnbinom
        cx = mp.fsum(mp.log(theta + i) for i in range(x)) - mp.loggamma(x + 1)
        lam = mp.exp(failr)
        fp = -lam + x * mp.log(lam) - mp.loggamma(x + 1)
        ninf = mp.mpf("-inf")
        la, lb = [], []
        for k in range(G):
            m = mp.mpf(float(mag[k]))
            mu = mp.mpf(x) if k in over else mp.exp(m * corra + corrb)
            lp = -mp.log1p(mu / theta)
            if x == 0:
                nb = theta * lp
            elif mu == 0:
                nb = ninf
            else:
                nb = cx + theta * lp + x * (-mp.log1p(theta / mu))
            z = m * conca + concb
            l1 = mp.log1p(mp.exp(z))  # log cfp = -l1, log(1 - cfp) = z - l1
            la.append(nb + z - l1)
            lb.append(fp - l1)
        mx = max(max(la), max(lb))
        e = [mp.exp(a - mx) + mp.exp(b - mx) for a, b in zip(la, lb)]
        s = mp.fsum(e)
        mlp = mp.mpf(float(minlogprob))
        out = []
        for k in range(G):
            t = mp.log(e[k] / s) if e[k] > 0 else ninf
            cl = bool(clamped[k]) if clamped is not None else t < mlp
            out.append(mlp if cl else t)
        return out


def exact_rows(model_row, ucl_c, uci_c, mag, ref_post_c, minlogprob, ncols=None):
    """column() for `ncols` of one cell's unique counts (the smallest, the largest and evenly spaced
    ranks between; None: all), with the oracle's clamp decisions read off its table ref_post_c
    (genes x grid): [(gene row showing that count, exact T)]."""
    u = np.asarray(ucl_c)
    order = np.argsort(u)
    pick = order if ncols is None else order[np.unique(np.linspace(0, len(u) - 1, ncols).round().astype(int))]
    out = []
    for j in pick:
        gene = int(np.nonzero(np.asarray(uci_c) == j)[0][0])
        row = ref_post_c[gene]
        out.append((gene, column(model_row, mag, int(u[j]), minlogprob, clamped=(row == minlogprob))))
    return out


def max_error(post_c, exact, rtol, atol, margin_abs=0.0):
    """Over the exact rows: max |post - exact|, and the largest ratio of |post - exact| to
    margin_abs + rtol |exact| + atol."""
    worst = ratio = 0.0
    for gene, ex in exact:
        err = np.array(abs_errors(post_c[gene], ex))
        bar = margin_abs + rtol * np.abs(np.array([float(v) for v in ex])) + atol
        worst, ratio = max(worst, float(err.max())), max(ratio, float((err / bar).max()))
    return worst, ratio


def abs_errors(values, exact):
    """|values_k - exact_k| as floats (the difference formed at 60 digits)."""
    with mp.workdps(DPS):
        return [float(abs(mp.mpf(float(v)) - e)) for v, e in zip(values, exact)]
