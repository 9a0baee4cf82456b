"""Plain numpy restatements for scde.error.models (float64, one cell at a time); the reference
of tests/test_error_models.py and tests/test_gpu_error_models.py.

  * the *literal* input stage: R's per-pair lists (``vi``, ``clusters``, ``posterior``) under
    threshold segmentation, and ``vil``, ``vi``, ``fpm``, ``cp`` derived from them as
    R/functions.R:3030-3039 and 3253-3303 read (``%in%``, ``rowMeans(log(...), na.rm = TRUE)``);
  * the closed forms DESIGN.md section 4.16 states for the same quantities;
  * ``fit_cell_nb2``: the project's contract for fit.nb2.mixture.model (R/functions.R:3630-3651,
    4002-4010, 4434-4547, 4549-4820, MASS::theta.ml), step by step as section 4.16 states it.

Sums are numpy's; the GPU's fixed-order sums differ from them by rounding.  The densities, the
Cholesky solve and log_sigmoid are tests/knn_fit_ref.py's.
"""
import functools
import itertools
import math

import numpy as np
from scipy.special import digamma, gammaln, polygamma

import knn_fit_ref as F

THRESHOLD_PRIOR = 1 - 1e-6
EPS = float(np.finfo(np.float64).eps)
OK, TOO_FEW, NO_WEIGHT, NOT_FINITE, IRLS_FAILED = 0, 1, 2, 3, 5


# ================================================================== the literal input stage
def combn_pairs(ids):
    """R's combn(ids, 2), as a list of pairs."""
    return list(itertools.combinations(ids, 2))


def crossfit_pair(counts, i, j, thr):
    """One pair's ``rli`` under threshold.segmentation (R/functions.R:2991-2992, 3030-3039);
    ``vi`` holds 0-based rows."""
    c1, c2 = counts[:, i], counts[:, j]
    vi = np.flatnonzero(c1 + c2 > 0)
    cl = np.full(len(vi), 2)
    cl[c1[vi] < thr] = 1
    cl[c2[vi] < thr] = 3
    cl[(c1[vi] < thr) & (c2[vi] < thr)] = 0
    tp = THRESHOLD_PRIOR
    pm = np.column_stack([np.where(cl == 1, tp, 1 - tp), np.where(cl == 3, tp, 1 - tp)])
    return {"ii": (i, j), "clusters": cl, "posterior": pm, "vi": vi}


def literal_inputs(counts, ids, pairs, ls, thr, min_nonfailed):
    """One group's ``vil`` (genes x len(ids); a cell in no pair has an all-False column, R's
    tapply over an empty level aside), and per cell of the group ``vi``, ``fpm`` and ``cp[, 1]``
    (NaN outside vi), from the per-pair lists as calculate.individual.models builds them."""
    counts = np.asarray(counts)
    N = counts.shape[0]
    rows = np.arange(N)
    rl = [crossfit_pair(counts, i, j, thr) for i, j in pairs]
    per_cell = {c: [] for c in ids}
    for d in rl:
        per_cell[d["ii"][0]].append(~np.isin(rows, d["vi"][d["clusters"] > 1]))
        per_cell[d["ii"][1]].append(~np.isin(rows, d["vi"][d["clusters"] % 3 != 0]))
    vil = np.zeros((N, len(ids)), bool)
    for k, c in enumerate(ids):
        if per_cell[c]:
            vil[:, k] = np.sum(np.column_stack(per_cell[c]), axis=1) == 0
    out = {"vil": vil, "vi": np.zeros((N, len(ids)), bool), "fpm": np.full((N, len(ids)), np.nan),
           "fail_prior": np.full((N, len(ids)), np.nan), "nabove": np.zeros((N, len(ids)), np.int64)}
    for k, c in enumerate(ids):
        others = [m for m in range(len(ids)) if m != k]
        nab = vil[:, others].sum(axis=1)
        out["nabove"][:, k] = nab
        vi = np.flatnonzero(nab >= min(len(ids) - 1, min_nonfailed))
        oc = [ids[m] for m in others]
        fpm = np.mean(counts[np.ix_(vi, oc)] / ls[oc][None, :], axis=1) if oc else np.full(len(vi), np.nan)
        cols = []
        for d in rl:
            for side in (0, 1):
                if d["ii"][side] == c:
                    ivi = np.full(N, -1)
                    ivi[d["vi"]] = np.arange(len(d["vi"]))
                    col = np.full(len(vi), np.nan)
                    has = ivi[vi] >= 0
                    col[has] = d["posterior"][ivi[vi][has], side]
                    cols.append(col)
        if cols:
            lg = np.log(np.column_stack(cols))
            cnt = np.sum(~np.isnan(lg), axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                cp = np.exp(np.nansum(lg, axis=1) / cnt)
        else:
            cp = np.full(len(vi), np.nan)
        cp[np.isnan(cp)] = 1 - 1e-10
        out["vi"][vi, k] = True
        out["fpm"][vi, k] = fpm
        out["fail_prior"][vi, k] = cp
    return out


def closed_inputs(counts, ids, pairs, ls, thr, min_nonfailed):
    """The same quantities by section 4.16's closed forms."""
    counts = np.asarray(counts)
    N = counts.shape[0]
    in_pair = {c: False for c in ids}
    partners = {c: [] for c in ids}
    for i, j in pairs:
        in_pair[i] = in_pair[j] = True
        partners[i].append(j)
        partners[j].append(i)
    vil = np.column_stack([(counts[:, c] >= thr) & in_pair[c] for c in ids])
    out = {"vil": vil, "vi": np.zeros((N, len(ids)), bool), "fpm": np.full((N, len(ids)), np.nan),
           "fail_prior": np.full((N, len(ids)), np.nan), "nabove": np.zeros((N, len(ids)), np.int64)}
    hi, lo = math.log(THRESHOLD_PRIOR), math.log(1 - THRESHOLD_PRIOR)  # (1 - (1 - 1e-6) is not 1e-6 in double)
    for k, c in enumerate(ids):
        others = [m for m in range(len(ids)) if m != k]
        nab = vil[:, others].sum(axis=1)
        vi = nab >= min(len(ids) - 1, min_nonfailed)
        fpm = np.zeros(N)
        for m in others:
            fpm = fpm + counts[:, ids[m]] / ls[ids[m]]
        fpm = fpm / len(others) if others else np.full(N, np.nan)
        s = np.zeros(N)
        cnt = np.zeros(N)
        for j in partners[c]:
            seen = counts[:, c] + counts[:, j] > 0
            high = (counts[:, c] < thr) & (counts[:, j] >= thr)
            s = s + np.where(seen, np.where(high, hi, lo), 0.0)
            cnt = cnt + seen
        with np.errstate(invalid="ignore", divide="ignore"):
            cp = np.where(cnt > 0, np.exp(s / cnt), 1 - 1e-10)
        out["nabove"][:, k] = nab
        out["vi"][:, k] = vi
        out["fpm"][vi, k] = fpm[vi]
        out["fail_prior"][vi, k] = cp[vi]
    return out


def model_inputs(counts, codes, pairs, ls, thr, min_nonfailed, literal=False):
    """genes x cells ``vi``, ``nabove``, ``fpm``, ``fail_prior`` over all groups (``codes``: one
    integer per cell; ``pairs``: 2 x P cell indices)."""
    counts = np.asarray(counts)
    N, C = counts.shape
    out = {"vi": np.zeros((N, C), bool), "nabove": np.zeros((N, C), np.int64), "fpm": np.full((N, C), np.nan),
           "fail_prior": np.full((N, C), np.nan)}
    plist = [(int(a), int(b)) for a, b in np.asarray(pairs).T]
    for g in np.unique(codes):
        ids = [int(c) for c in np.flatnonzero(codes == g)]
        gp = [p for p in plist if codes[p[0]] == g]
        r = (literal_inputs if literal else closed_inputs)(counts, ids, gp, np.asarray(ls, np.float64), thr,
                                                           min_nonfailed)
        for k in out:
            out[k][:, ids] = r[k]
    return out


# ================================================================== the fit
def link_mu(eta):
    """The log link's linkinv (and mu.eta): pmax(exp(eta), .Machine$double.eps)."""
    with np.errstate(over="ignore"):
        return np.maximum(np.exp(eta), EPS)


def deviance(y, mu, wt, theta):
    """sum(dev.resids): Poisson when theta is None, MASS's negative.binomial(theta) otherwise."""
    with np.errstate(all="ignore"):
        if theta is None:
            r = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0) / mu) - (y - mu), mu)
        else:
            r = y * np.log(np.maximum(1.0, y) / mu) - (y + theta) * np.log((y + theta) / (mu + theta))
        return float(np.sum(2.0 * wt * r))


def irls(y, l, wt, eta, theta, maxit):
    """custom.glm.fit with the design [1, l] and the log link, on the genes the caller passed (all
    of positive weight), from the per-gene linear predictor ``eta``.  (coef, status)."""
    eps = 1e-8
    dev_old = deviance(y, link_mu(eta), wt, theta)
    if not np.isfinite(dev_old):
        return None, IRLS_FAILED
    coef_old = None
    start = None
    for _ in range(maxit):
        mu = link_mu(eta)
        with np.errstate(all="ignore"):
            var = mu if theta is None else mu + mu * mu / theta
            W = wt * (mu * mu) / var
            z = eta + (y - mu) / mu
        A = np.array([[np.sum(W), np.sum(W * l)], [np.sum(W * l), np.sum(W * l * l)]])
        g = np.array([np.sum(W * z), np.sum(W * l * z)])
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(g))):
            return None, IRLS_FAILED
        start = F.chol_solve(A, g)
        if not np.all(np.isfinite(start)):
            return None, IRLS_FAILED
        dev = deviance(y, link_mu(start[0] + start[1] * l), wt, theta)
        if not np.isfinite(dev):
            if coef_old is None:
                return None, IRLS_FAILED
            ii = 1
            while not np.isfinite(dev):
                if ii > maxit:
                    return None, IRLS_FAILED
                ii += 1
                start = (start + coef_old) / 2
                dev = deviance(y, link_mu(start[0] + start[1] * l), wt, theta)
        if coef_old is not None and (dev - dev_old) / (0.1 + abs(dev)) > 3 * eps:
            ii = 1
            while (dev - dev_old) / (0.1 + abs(dev)) > 3 * eps:
                if ii > maxit:
                    break
                ii += 1
                start = (start + coef_old) / 2
                dev = deviance(y, link_mu(start[0] + start[1] * l), wt, theta)
        eta = start[0] + start[1] * l
        if abs(dev - dev_old) / (0.1 + abs(dev)) < eps:
            break
        dev_old = dev
        coef_old = start
    return start, OK


def theta_ml(y, mu, wt):
    """MASS::theta.ml(y, mu, sum(wt), wt, limit = 20); the result is abs(t0)."""
    n = np.sum(wt)
    with np.errstate(all="ignore"):
        t0 = n / np.sum(wt * (y / mu - 1.0) ** 2)
        it, dl = 0, 1.0
        while True:
            it += 1
            if not (it < 20 and abs(dl) > EPS ** 0.25):
                break
            t0 = abs(t0)
            score = np.sum(wt * (digamma(t0 + y) - digamma(t0) + math.log(t0) + 1.0 - np.log(t0 + mu)
                                 - (y + t0) / (mu + t0)))
            info = np.sum(wt * (-polygamma(1, t0 + y) + polygamma(1, t0) - 1.0 / t0 + 2.0 / (mu + t0)
                                - (y + t0) / (mu + t0) ** 2))
            dl = score / info
            t0 = t0 + dl
    return abs(float(t0))


def nb_loglik(y, mu, wt, th):
    with np.errstate(all="ignore"):
        return float(np.sum(wt * (gammaln(th + y) - gammaln(th) - gammaln(y + 1.0) + th * math.log(th)
                                  + y * np.log(mu + (y == 0)) - (th + y) * np.log(th + mu))))


def glm_nb_fit(y, l, wt, init_theta, theta_lo, theta_hi):
    """glm.nb.fit on the genes of positive weight.  (coef, theta, status)."""
    keep = wt > 0
    y, l, wt = y[keep], l[keep], wt[keep]
    if len(y) < 1:
        return None, np.nan, NO_WEIGHT
    clamp = lambda t: min(max(t, theta_lo), theta_hi)  # (a NaN passes through)
    if init_theta is None:
        eta = np.log(y + 0.1)
    else:
        eta = np.log(y + (y == 0) / 6.0)
    coef, st = irls(y, l, wt, eta, init_theta, 20)
    if st != OK:
        return None, np.nan, st
    eta = coef[0] + coef[1] * l
    th = theta_ml(y, link_mu(eta), wt)
    if not np.isfinite(th):
        return None, np.nan, NOT_FINITE
    th = clamp(th)
    d1 = math.sqrt(2.0 * max(1, len(y) - 2))
    dl = 1.0
    lm = nb_loglik(y, link_mu(eta), wt, th)
    lm0 = lm + 2 * d1
    it = 0
    while True:
        it += 1
        if not (it <= 20 and abs(lm0 - lm) / d1 + abs(dl) > 1e-8):
            break
        t0 = th
        th = theta_ml(y, link_mu(eta), wt)  # (from the mu before this round's refit, as R)
        if not np.isfinite(th):
            return None, np.nan, NOT_FINITE
        th = clamp(th)
        coef, st = irls(y, l, wt, eta, t0, 200)
        if st != OK:
            return None, np.nan, st
        eta = coef[0] + coef[1] * l
        dl = t0 - th
        lm0 = lm
        lm = nb_loglik(y, link_mu(eta), wt, th)
    if not (np.isfinite(lm) and np.all(np.isfinite(coef))):
        return None, np.nan, NOT_FINITE
    return coef, th, OK


def concomitant2(l, p2):
    """(b0, b1) maximising sum p2 log s(eta) + (1 - p2) log(1 - s(eta)), eta = b0 + b1 l: the
    Newton of knn_fit_ref.concomitant on two parameters."""
    beta = np.zeros(2)
    z = np.stack([np.ones_like(l), l])

    def obj(b):
        eta = b[0] + b[1] * l
        return float(np.sum(p2 * F.log_sigmoid(eta) + (1 - p2) * F.log_sigmoid(-eta)))
    f = obj(beta)
    for _ in range(50):
        eta = beta[0] + beta[1] * l
        lsp, lsn = F.log_sigmoid(eta), F.log_sigmoid(-eta)
        g = z @ (p2 * np.exp(lsn) - (1 - p2) * np.exp(lsp))
        H = (z * np.exp(lsp + lsn)) @ z.T
        d = F.chol_solve(H, g)
        if not np.all(np.isfinite(d)):
            return np.full(2, np.nan)
        t = 1.0
        for _h in range(30):
            fb = obj(beta + t * d)
            if np.isfinite(fb) and fb >= f - 1e-10 * (abs(f) + 1.0):
                break
            t *= 0.5
        else:
            return np.full(2, np.nan)
        step = t * d
        beta = beta + step
        f = fb
        if np.max(np.abs(step)) / (1 + np.max(np.abs(beta))) < 1e-10:
            return beta
    return np.full(2, np.nan)


def fit_cell_nb2(y, x, fp, iter=50, background_rate=0.1):
    """One cell's fit.  y: counts of the valid genes, x: their fpm (> 0), fp: the starting
    failed-component posteriors.  Returns a dict: ``row`` (12 values in knn_fit_ref.COLUMNS' order,
    the last six NaN; all NaN where the status is not 0), ``iterations``, ``llh``, ``status``,
    ``clusters`` (1 / 2), ``p1``, and ``refit`` (whether the underfit refit ran)."""
    y = np.asarray(y, np.float64)
    x = np.asarray(x, np.float64)
    n = len(y)
    row = np.full(12, np.nan)
    out = {"row": row, "iterations": 0, "llh": np.nan, "status": OK, "clusters": np.zeros(n, np.int32),
           "p1": np.full(n, np.nan), "refit": False, "negative_slope": False}
    if n < 3:
        out["status"] = TOO_FEW
        return out
    with np.errstate(divide="ignore"):
        l = np.log(x)
    p1 = np.asarray(fp, np.float64).copy()
    p2 = 1.0 - p1
    llh_old, llh, status, its = -np.inf, np.nan, OK, 0
    beta = coef = None
    theta = np.nan
    for its in range(1, int(iter) + 1):
        beta = concomitant2(l, p2)
        if not np.all(np.isfinite(beta)):
            status = NOT_FINITE
            break
        wt = np.where(y <= 1, p2 / 1e6, p2)
        coef, theta, status = glm_nb_fit(y, l, wt, None, 0.5, np.inf)
        if status != OK:
            break
        out["negative_slope"] = bool(coef[1] < 0)
        if coef[1] < 0:  # R's "ugly hack": the intercept is a mean, not its log
            coef = np.array([np.sum(y * wt) / n / np.sum(wt), 0.0])
        if not np.all(np.isfinite(coef)):
            status = NOT_FINITE
            break
        eta = beta[0] + beta[1] * l
        mu = link_mu(coef[0] + coef[1] * l)
        with np.errstate(all="ignore"):
            a1 = F.log_sigmoid(-eta) + F.dpois_log(y, background_rate)
            a2 = F.log_sigmoid(eta) + F.dnbinom_log(y, theta, theta / (theta + mu))
            m = np.maximum(a1, a2)
            lse = m + np.log(np.exp(a1 - m) + np.exp(a2 - m))
            p1, p2 = np.exp(a1 - lse), np.exp(a2 - lse)
        llh = float(np.sum(lse))
        if not np.isfinite(llh):
            status = NOT_FINITE
            break
        if abs(llh - llh_old) / (abs(llh) + 0.1) < 1e-6:
            break
        llh_old = llh
    if status == OK and theta == 0.5:
        out["refit"] = True
        coef, theta, status = glm_nb_fit(y, l, (p2 > p1).astype(np.float64), 0.5, 0.0, 1e5)
        if status == OK and not (theta > 0):
            status = NOT_FINITE
    out["iterations"], out["status"] = its, status
    if status != OK:
        return out
    row[:6] = [beta[0], beta[1], math.log(background_rate), coef[0], coef[1], theta]
    out["llh"] = llh
    out["clusters"] = np.where(p2 > p1, 2, 1).astype(np.int32)
    out["p1"] = p1
    return out


# ================================================================== synthetic cells
def synthetic_cell_nb2(n, seed, kind="plain"):
    """(count, fpm, fail prior) of one cell: log-normal fpm, an NB(theta) correlated component of
    mean exp(c0) fpm^c1, a logistic drop-out, and starting posteriors as the threshold
    segmentation gives (high where the count is below 4 and the magnitude is not small).
    ``kind``: "plain"; "negative" (counts fall with the magnitude: the negative-slope rule);
    "underfit" (an over-dispersed component: theta clamps at 0.5); "large" (counts of 1e5);
    "sparse" (all but three genes at y <= 1)."""
    rng = np.random.default_rng(seed)
    x = np.exp(rng.normal(2.0, 1.6, n))
    l = np.log(x)
    c0, c1, th = rng.normal(0.5, 0.2), rng.uniform(0.6, 1.0), math.exp(rng.normal(0.5, 0.4))
    if kind == "negative":
        c0, c1 = 4.0, -0.4
    if kind == "underfit":
        th = 0.05
    if kind == "large":
        c0 += math.log(1e5) - 2.0
    mu = np.exp(c0 + c1 * l)
    y = rng.negative_binomial(th, th / (th + mu)).astype(np.float64)
    fail = rng.random(n) < 1 / (1 + np.exp(-1.0 + 1.2 * l))
    y[fail] = rng.poisson(0.1, int(fail.sum()))
    if kind == "sparse":
        keep = np.argsort(-y, kind="stable")[:3]
        top = y[keep]
        y = np.minimum(y, 1.0)
        y[keep] = np.maximum(top, 5.0)
    fp = np.where((y < 4) & (x >= np.median(x)), THRESHOLD_PRIOR, 1 - THRESHOLD_PRIOR)
    fp = np.where(rng.random(n) < 0.3, np.exp(0.5 * (np.log(fp) + math.log(1e-6))), fp)  # (a mean of both levels)
    y = np.minimum(y, 2.0 ** 30).astype(np.int32)
    return y, x, fp


ROW_COLS = [0, 1, 3, 4, 5]


def row_spread(r, q):
    """Per quantity: conc.b, conc.a, corr.b, corr.a relative to max(1, |.|); theta relative."""
    d = {c: abs(q[c] - r[c]) / max(1.0, abs(r[c])) for c in (0, 1, 3, 4)}
    d[5] = abs(q[5] - r[5]) / abs(r[5])
    return d


@functools.lru_cache(maxsize=None)
def reference_nb2(n, seed, kind="plain", iter=50, permutations=0):
    """The generator's cell and its fit, computed once per session; with ``permutations`` also the
    restatement's own spread over that many gene permutations: ``spread`` (per column of
    ROW_COLS), ``llh_spread`` (relative), ``p1_spread`` (absolute), ``stable`` (the same status,
    iterations and branches in every permutation)."""
    cell = synthetic_cell_nb2(n, seed, kind)
    y, x, fp = cell
    fit = fit_cell_nb2(y, x, fp, iter=iter)
    out = {"cell": cell, "fit": fit, "spread": {c: 0.0 for c in ROW_COLS}, "llh_spread": 0.0, "p1_spread": 0.0,
           "stable": True}
    for s in range(1, permutations + 1):
        o = np.random.default_rng(s).permutation(len(y))
        p = fit_cell_nb2(y[o], x[o], fp[o], iter=iter)
        same = all(p[k] == fit[k] for k in ("status", "iterations", "refit", "negative_slope"))
        out["stable"] = out["stable"] and same
        if not same or fit["status"] != OK:
            continue
        for c, v in row_spread(fit["row"], p["row"]).items():
            out["spread"][c] = max(out["spread"][c], v)
        out["llh_spread"] = max(out["llh_spread"], abs(p["llh"] - fit["llh"]) / abs(fit["llh"]))
        back = np.empty(len(y))
        back[o] = p["p1"]
        out["p1_spread"] = max(out["p1_spread"], float(np.max(np.abs(back - fit["p1"]))))
    return out
