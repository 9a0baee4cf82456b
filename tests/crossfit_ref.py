"""Plain numpy restatements for the mixture cross-fit of cell pairs (scde.error.models with
threshold.segmentation = FALSE), written from DESIGN.md section 4.19 and R/functions.R:2993-3028,
3147-3155, 3253-3303; the reference of tests/test_crossfit.py and tests/test_gpu_crossfit.py.

  * ``fit_pair``: the project's statement of flexmix's EM for one pair, step by step;
  * ``crossfit``: all pairs, in ``crossfit_models``' shape;
  * ``literal_reduce``: R's list code from per-pair lists to ``vil``, ``vi``, ``fpm``, ``cp``
    (``%in%``, ``rowSums``, ``rowMeans(log())``), and ``reduce``: section 4.19's statement of it.

glm.nb.fit is tests/error_models_ref.py's; the densities, the Cholesky solve and the sums are as
there (numpy's sums: the GPU's fixed-order sums differ from them by rounding).
"""
import numpy as np

import error_models_ref as E
import knn_fit_ref as F

OK, NO_ROWS, NO_WEIGHT, NOT_FINITE, IRLS_FAILED, LOST = 0, 1, 2, 3, 5, 6


# ================================================================== stage 1: one pair's EM
def log_pi3(b, x):
    """log softmax(0, b0 + b1 x, b2 + b3 x) by a max-shifted log-sum-exp: 3 x rows."""
    e2, e3 = b[0] + b[1] * x, b[2] + b[3] * x
    m = np.maximum(0.0, np.maximum(e2, e3))
    with np.errstate(all="ignore"):
        lse = m + np.log(np.exp(-m) + np.exp(e2 - m) + np.exp(e3 - m))
    return np.stack([-lse, e2 - lse, e3 - lse])


def concomitant3(x, p):
    """(a2, b2, a3, b3) maximising sum_i sum_k p_ik log pi_ik: error_models_ref.concomitant2's
    Newton on four parameters.  p: 3 x rows.  NaN on failure."""
    beta = np.zeros(4)

    def obj(b):
        return float(np.sum(p * log_pi3(b, x)))
    f = obj(beta)
    for _ in range(50):
        q = np.exp(log_pi3(beta, x))
        g2 = p[1] * (q[0] + q[2]) - (p[0] + p[2]) * q[1]
        g3 = p[2] * (q[0] + q[1]) - (p[0] + p[1]) * q[2]
        h22, h33, h23 = q[1] * (q[0] + q[2]), q[2] * (q[0] + q[1]), -(q[1] * q[2])
        g = np.array([np.sum(g2), np.sum(x * g2), np.sum(g3), np.sum(x * g3)])

        def blk(h):
            return np.sum(h), np.sum(x * h), np.sum(x * h * x)
        a, b, c = blk(h22), blk(h23), blk(h33)
        H = np.array([[a[0], a[1], b[0], b[1]],
                      [a[1], a[2], b[1], b[2]],
                      [b[0], b[1], c[0], c[1]],
                      [b[1], b[2], c[1], c[2]]])
        d = F.chol_solve(H, g)
        if not np.all(np.isfinite(d)):
            return np.full(4, np.nan)
        t = 1.0
        for _h in range(30):
            fb = obj(beta + t * d)
            if np.isfinite(fb) and fb >= f - 1e-10 * (abs(f) + 1.0):
                break
            t *= 0.5
        else:
            return np.full(4, np.nan)
        step = t * d
        beta = beta + step
        f = fb
        if np.max(np.abs(step)) / (1 + np.max(np.abs(beta))) < 1e-10:
            return beta
    return np.full(4, np.nan)


def fit_driver(y, l, p2):
    """One NB driver of component 2: (coef, theta, status)."""
    n = len(y)
    wt = np.where(y <= 1, p2 / 1e6, p2)
    try:
        coef, theta, st = E.glm_nb_fit(y, l, wt, None, 0.0, 1e3)
    except ValueError:  # (math.log(0): theta clamped to 0, the kernel's NaN log-likelihood)
        return None, np.nan, NOT_FINITE
    if st != OK:
        return None, np.nan, st
    if coef[1] < 0:
        with np.errstate(all="ignore"):
            coef = np.array([np.sum(y * wt) / n / np.sum(wt), 0.0])
    if not np.all(np.isfinite(coef)):
        return None, np.nan, NOT_FINITE
    return coef, theta, OK


def fit_pair(c1, c2, thr=4, min_prior=1e-5, zero_lambda=0.1, iter=200):
    """One pair's fit.  c1, c2: the two cells' counts over all genes.  Returns a dict: ``status``,
    ``iterations``, ``llh``, ``params`` (10; NaN unless status 0), ``rows`` (0-based genes),
    ``clusters`` (genes; 0 outside the rows or on failure), ``posterior`` (genes x 3; NaN likewise)."""
    c1, c2 = np.asarray(c1), np.asarray(c2)
    N = len(c1)
    rows = np.flatnonzero(c1.astype(np.int64) + c2 > 0)
    out = {"status": OK, "iterations": 0, "llh": np.nan, "params": np.full(10, np.nan), "rows": rows,
           "clusters": np.zeros(N, np.int8), "posterior": np.full((N, 3), np.nan)}
    n = len(rows)
    if n < 1:
        out["status"] = NO_ROWS
        return out
    y1, y2 = c1[rows].astype(np.float64), c2[rows].astype(np.float64)
    l1, l2 = np.log(y1 + 1.0), np.log(y2 + 1.0)
    x = (l1 + l2) / 2.0
    ind = np.stack([y1 <= thr, (y1 > thr) & (y2 > thr), y2 <= thr]).astype(np.float64)
    p = ind / ind.sum(axis=0)
    llh_old, llh, status, its = -np.inf, np.nan, OK, 0
    for its in range(1, int(iter) + 1):
        if not np.all(p.sum(axis=1) / n >= min_prior):
            status = LOST
            break
        beta = concomitant3(x, p)
        if not np.all(np.isfinite(beta)):
            status = NOT_FINITE
            break
        ca, tha, status = fit_driver(y1, l2, p[1])
        if status != OK:
            break
        cb, thb, status = fit_driver(y2, l1, p[1])
        if status != OK:
            break
        lp = log_pi3(beta, x)
        mua, mub = E.link_mu(ca[0] + ca[1] * l2), E.link_mu(cb[0] + cb[1] * l1)
        with np.errstate(all="ignore"):
            a = np.stack([lp[0] + F.dpois_log(y1, zero_lambda),
                          lp[1] + F.dnbinom_log(y1, tha, tha / (tha + mua)) + F.dnbinom_log(y2, thb, thb / (thb + mub)),
                          lp[2] + F.dpois_log(y2, zero_lambda)])
            m = a.max(axis=0)
            lse = m + np.log(np.exp(a[0] - m) + np.exp(a[1] - m) + np.exp(a[2] - m))
            p = np.exp(a - lse)
        llh = float(np.sum(lse))
        if not np.isfinite(llh):
            status = NOT_FINITE
            break
        if abs(llh - llh_old) / (abs(llh) + 0.1) < 1e-6:
            break
        llh_old = llh
    out["iterations"], out["status"] = its, status
    if status != OK:
        return out
    out["llh"] = llh
    out["params"] = np.array([*beta, ca[0], ca[1], tha, cb[0], cb[1], thb])
    out["clusters"][rows] = np.argmax(p, axis=0) + 1  # (the first of equal maxima)
    out["posterior"][rows] = p.T
    return out


def crossfit(counts, pairs, **kw):
    """Every pair's fit in ``crossfit_models``' shape, and the per-pair dicts under ``"fits"``."""
    counts = np.asarray(counts)
    fits = [fit_pair(counts[:, i], counts[:, j], **kw) for i, j in np.asarray(pairs).T]
    return {"pairs": np.asarray(pairs, np.int32),
            "status": np.array([f["status"] for f in fits], np.int32),
            "iterations": np.array([f["iterations"] for f in fits], np.int32),
            "llh": np.array([f["llh"] for f in fits]),
            "params": np.array([f["params"] for f in fits]).reshape(len(fits), 10),
            "clusters": np.stack([f["clusters"] for f in fits], axis=1),
            "posterior": np.stack([f["posterior"][:, [0, 2]].T for f in fits], axis=2),
            "fits": fits}


# ================================================================== stage 2
def pair_lists(cf):
    """R's ``cfm``: per status-0 pair ``ii``, ``vi`` (the rows: the posterior is not NaN),
    ``clusters`` and ``posterior`` (rows x 2) over them.  A failed pair is not in the list, as in R."""
    out = []
    for p in range(cf["pairs"].shape[1]):
        if cf["status"][p] != 0:
            continue
        vi = np.flatnonzero(~np.isnan(cf["posterior"][0, :, p]))
        out.append({"ii": (int(cf["pairs"][0, p]), int(cf["pairs"][1, p])), "vi": vi,
                    "clusters": np.asarray(cf["clusters"][vi, p], np.int64),
                    "posterior": np.column_stack([cf["posterior"][0, vi, p], cf["posterior"][1, vi, p]])})
    return out


def literal_reduce(counts, ids, rl, ls, min_nonfailed):
    """One group's ``vil``, and per cell ``nabove``, ``vi``, ``fpm`` and ``cp[, 1]`` from the
    per-pair lists, as R/functions.R:3253-3303 reads.  R's cbind puts a cell's first-cell pairs
    before its second-cell pairs; a mean of logs does not depend on that but for rounding."""
    counts = np.asarray(counts)
    N = counts.shape[0]
    genes = np.arange(N)
    per_cell = {c: [] for c in ids}
    for d in rl:
        if d["ii"][0] in per_cell:
            per_cell[d["ii"][0]].append(~np.isin(genes, d["vi"][d["clusters"] > 1]))
            per_cell[d["ii"][1]].append(~np.isin(genes, d["vi"][d["clusters"] % 3 != 0]))
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
        fpm = np.mean(counts[np.ix_(vi, oc)] / ls[oc][None, :], axis=1)
        cols = []
        for side in (0, 1):
            for d in rl:
                if d["ii"][side] == c:
                    ivi = np.full(N, -1)
                    ivi[d["vi"]] = np.arange(len(d["vi"]))
                    col = np.full(len(vi), np.nan)
                    has = ivi[vi] >= 0
                    col[has] = d["posterior"][ivi[vi][has], side]
                    cols.append(col)
        if cols:
            with np.errstate(invalid="ignore", divide="ignore"):
                lg = np.log(np.column_stack(cols))
                cnt = np.sum(~np.isnan(lg), axis=1)
                cp = np.exp(np.nansum(lg, axis=1) / cnt)
        else:
            cp = np.full(len(vi), np.nan)
        cp[np.isnan(cp)] = 1 - 1e-10
        out["vi"][vi, k] = True
        out["fpm"][vi, k] = fpm
        out["fail_prior"][vi, k] = cp
    return out


def reduce_group(counts, ids, cf, ls, min_nonfailed):
    """The same quantities as section 4.19 states them, from ``crossfit_models``' arrays."""
    counts = np.asarray(counts)
    N = counts.shape[0]
    pairs, status = np.asarray(cf["pairs"]), np.asarray(cf["status"])
    cl, post = np.asarray(cf["clusters"]), np.asarray(cf["posterior"])
    vil = np.zeros((N, len(ids)), bool)
    logsum = np.zeros((N, len(ids)))
    cnt = np.zeros((N, len(ids)), np.int64)
    for k, c in enumerate(ids):
        nok = 0
        good = np.ones(N, bool)
        for p in range(pairs.shape[1]):  # the pairs' order
            for side in (0, 1):
                if pairs[side, p] != c or status[p] != 0:
                    continue
                nok += 1
                k_p = cl[:, p]
                good &= ((k_p >= 2) if side == 0 else ((k_p >= 1) & (k_p <= 2)))
                row = ~np.isnan(post[side, :, p])
                with np.errstate(divide="ignore"):
                    logsum[row, k] = logsum[row, k] + np.log(post[side, row, p])
                cnt[row, k] += 1
        vil[:, k] = good & (nok > 0)
    out = {"vil": vil, "vi": np.zeros((N, len(ids)), bool), "fpm": np.full((N, len(ids)), np.nan),
           "fail_prior": np.full((N, len(ids)), np.nan), "nabove": np.zeros((N, len(ids)), np.int64)}
    for k, c in enumerate(ids):
        others = [m for m in range(len(ids)) if m != k]
        nab = vil[:, others].sum(axis=1)
        vi = nab >= min(len(ids) - 1, min_nonfailed)
        fpm = np.zeros(N)
        for m in others:
            fpm = fpm + counts[:, ids[m]] / ls[ids[m]]
        fpm = fpm / len(others)
        with np.errstate(invalid="ignore", divide="ignore"):
            cp = np.where(cnt[:, k] > 0, np.exp(logsum[:, k] / cnt[:, k]), 1 - 1e-10)
        out["nabove"][:, k] = nab
        out["vi"][:, k] = vi
        out["fpm"][vi, k] = fpm[vi]
        out["fail_prior"][vi, k] = cp[vi]
    return out


def reduce(counts, codes, cf, ls, min_nonfailed, literal=False):
    """genes x cells ``vil``, ``vi``, ``nabove``, ``fpm``, ``fail_prior`` over all groups."""
    counts = np.asarray(counts)
    N, C = counts.shape
    ls = np.asarray(ls, np.float64)
    out = {"vil": np.zeros((N, C), bool), "vi": np.zeros((N, C), bool), "nabove": np.zeros((N, C), np.int64),
           "fpm": np.full((N, C), np.nan), "fail_prior": np.full((N, C), np.nan)}
    rl = pair_lists(cf) if literal else None
    for g in np.unique(codes):
        ids = [int(c) for c in np.flatnonzero(codes == g)]
        r = literal_reduce(counts, ids, rl, ls, min_nonfailed) if literal else reduce_group(counts, ids, cf, ls,
                                                                                           min_nonfailed)
        for k in out:
            out[k][:, ids] = r[k]
    return out


def threshold_crossfit(counts, pairs, thr):
    """The clusters and posteriors the threshold rule gives (R/functions.R:3030-3037, t = 1 - 1e-6),
    in ``crossfit_models``' shape: the anchor that ties the reduction to scde_crossfit_inputs_*."""
    counts = np.asarray(counts)
    N, P = counts.shape[0], np.asarray(pairs).shape[1]
    cl = np.zeros((N, P), np.int8)
    post = np.full((2, N, P), np.nan)
    for p, (i, j) in enumerate(np.asarray(pairs).T):
        d = E.crossfit_pair(counts, i, j, thr)
        cl[d["vi"], p] = d["clusters"]
        post[0, d["vi"], p] = d["posterior"][:, 0]
        post[1, d["vi"], p] = d["posterior"][:, 1]
    return {"pairs": np.asarray(pairs, np.int32), "status": np.zeros(P, np.int32), "clusters": cl, "posterior": post}
