"""Plain numpy restatement of knn.error.models' neighbourhood stage (R/functions.R:1158-1237 and
estimate.library.sizes, 3141-3178), the reference of tests/test_knn.py and tests/test_gpu_knn.py.

Everything is float64 (the similarity also in np.longdouble, ``dtype=``), one cell and one gene
at a time where R is, with no shortcut the GPU code takes: values are sorted, not ranked through
a bit mask.  ``counts`` is genes x cells, ``thr`` min.count.threshold, valid = counts >= thr.
"""
import math

import numpy as np

TP = 1 - 1e-6  # threshold.prior


# ------------------------------------------------------------------ library sizes
def quantile7(x, p):
    """R's quantile(type = 7) of a vector."""
    x = np.sort(np.asarray(x, np.float64))
    h = (len(x) - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, len(x) - 1)
    return x[lo] + (h - lo) * (x[hi] - x[lo])


def average_rank(v):
    """R's rank(ties.method = "average"), 1-based."""
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    r = np.empty(len(v))
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and v[order[j + 1]] == v[order[i]]:
            j += 1
        r[order[i:j + 1]] = (i + j) / 2.0 + 1.0
        i = j + 1
    return r


def tmm_factor(obs, ref, n_o, n_r, logratio_trim=0.3, sum_trim=0.05, a_cutoff=-1e10):
    """One column's TMM factor against the reference column (Robinson & Oshlack 2010, with
    edgeR's documented defaults: weighted, trim 0.3 of M and 0.05 of A, A cutoff -1e10)."""
    obs, ref = np.asarray(obs, np.float64), np.asarray(ref, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_r = np.log2((obs / n_o) / (ref / n_r))
        abs_e = (np.log2(obs / n_o) + np.log2(ref / n_r)) / 2
        v = (n_o - obs) / n_o / obs + (n_r - ref) / n_r / ref
    fin = np.isfinite(log_r) & np.isfinite(abs_e) & (abs_e > a_cutoff)
    log_r, abs_e, v = log_r[fin], abs_e[fin], v[fin]
    if len(log_r) == 0 or np.max(np.abs(log_r)) < 1e-6:
        return 1.0
    n = len(log_r)
    lo_l = math.floor(n * logratio_trim) + 1
    hi_l = n + 1 - lo_l
    lo_s = math.floor(n * sum_trim) + 1
    hi_s = n + 1 - lo_s
    rl, rs = average_rank(log_r), average_rank(abs_e)
    keep = (rl >= lo_l) & (rl <= hi_l) & (rs >= lo_s) & (rs <= hi_s)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.sum(log_r[keep] / v[keep]) / np.sum(1 / v[keep])
    f = 2.0 ** f
    return 1.0 if np.isnan(f) else float(f)


def tmm_reference_column(x, lib):
    f75 = np.array([quantile7(x[:, j], 0.75) for j in range(x.shape[1])]) / lib
    if np.median(f75) < 1e-20:
        return int(np.argmax(np.sum(np.sqrt(x), axis=0)))
    return int(np.argmin(np.abs(f75 - np.mean(f75))))


def tmm_norm_factors(x):
    """TMM factors of the columns of x (rows x columns), scaled to a geometric mean of 1."""
    x = np.asarray(x, np.float64)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("x must be a matrix with at least one column")
    x = x[np.any(x != 0, axis=1)]
    C = x.shape[1]
    if x.shape[0] == 0 or C == 1:
        return np.ones(C)
    lib = x.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = tmm_reference_column(x, lib)
        f = np.array([tmm_factor(x[:, j], x[:, ref], lib[j], lib[ref]) for j in range(C)])
    return f / np.exp(np.mean(np.log(f)))


def library_size_genes(counts, min_size_entries=2000, thr=1):
    """gis of estimate.library.sizes with vil = counts >= thr (0-based, in R's order)."""
    counts = np.asarray(counts)
    N, C = counts.shape
    nv = (counts >= thr).sum(axis=1)
    if N < min_size_entries:
        raise ValueError(f"The number of valid genes ({N}) is lower then the specified min.size.entries "
                         f"({min_size_entries})")
    order = np.argsort(-nv, kind="stable")
    if nv[order[min_size_entries - 1]] < C:
        return order[:min_size_entries]
    return order[nv[order] == C]


def estimate_library_sizes(counts, min_size_entries=2000, thr=1, norm_factors=None):
    counts = np.asarray(counts)
    sub = counts[library_size_genes(counts, min_size_entries, thr)].astype(np.float64)
    f = tmm_norm_factors(sub) if norm_factors is None else np.asarray(norm_factors, np.float64)
    f = f / np.exp(np.mean(np.log(f)))  # (R divides calcNormFactors' result once more)
    return sub.sum(axis=0) * f / 1e6


# ------------------------------------------------------------------ similarity
def similarity(counts, thr=1, dtype=np.float64):
    """Pairwise-complete Pearson correlation of sqrt(counts) over counts >= thr, in the one-pass
    form of include/scde_hip.h (boot::corr with 0 / 1 weights), as the arithmetic gives it: NaN (0 / 0)
    where a pair has no common gene or a variance of exactly zero."""
    counts = np.asarray(counts)
    u = (counts >= thr).astype(dtype)
    x = np.where(counts >= thr, np.sqrt(np.maximum(counts, 0).astype(dtype)), dtype(0))
    xu, x2u = x * u, x * x * u
    s = u.T @ u
    with np.errstate(divide="ignore", invalid="ignore"):
        m1 = (xu.T @ u) / s
        m2 = m1.T
        cov = (xu.T @ xu) / s - m1 * m2
        v1 = (x2u.T @ u) / s - m1 * m1
        v2 = v1.T
        return cov / np.sqrt(v1 * v2)


def similarity_two_pass(counts, thr=1):
    """The same as stats::cor(use = "p") computes it: per pair, centred over the common genes."""
    counts = np.asarray(counts)
    N, C = counts.shape
    x = np.sqrt(np.maximum(counts, 0).astype(np.float64))
    ok = counts >= thr
    out = np.full((C, C), np.nan)
    for i in range(C):
        for j in range(C):
            m = ok[:, i] & ok[:, j]
            if m.sum() < 1:
                continue
            a, b = x[m, i] - x[m, i].mean(), x[m, j] - x[m, j].mean()
            den = math.sqrt(np.sum(a * a) * np.sum(b * b))
            if den > 0:
                out[i, j] = np.sum(a * b) / den
    return out


# ------------------------------------------------------------------ neighbours
def default_k(C):
    return int(np.round(C / 2))  # half to even, as R's round


def group_codes(groups, C):
    if groups is None:
        return np.zeros(C, np.int32)
    g = np.asarray(groups)
    if g.shape != (C,):
        raise ValueError("groups must have one entry per cell")
    return np.unique(g, return_inverse=True)[1].astype(np.int32)


def neighbour_order(row, cand):
    """The candidates in R's order(decreasing = TRUE): decreasing value, ties in index order,
    NaN last (in index order)."""
    cand = [int(j) for j in cand]
    real = sorted((j for j in cand if not np.isnan(row[j])), key=lambda j: (-row[j], j))
    return real + [j for j in cand if np.isnan(row[j])]


def neighbours(sim, k=None, groups=None):
    sim = np.asarray(sim, np.float64)
    C = sim.shape[0]
    k = default_k(C) if k is None else int(k)
    k = min(k, C - 1)
    g = group_codes(groups, C)
    kmax = max(min(k, int(np.max(np.bincount(g))) - 1), 0)
    out = np.full((C, kmax), -1, np.int32)
    for i in range(C):
        cand = [j for j in range(C) if j != i and g[j] == g[i]]
        o = neighbour_order(sim[i], cand)[:min(k, len(cand))]
        out[i, :len(o)] = o
    return out


# ------------------------------------------------------------------ expected magnitudes
def trimmed_mean(values, trim):
    """R's mean(x, trim =) of a vector without NA; NaN for an empty one."""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    if n == 0:
        return np.nan
    if trim >= 0.5:
        h = (n + 1) // 2
        return float(v[h - 1]) if n % 2 else float((v[h - 1] + v[h]) / 2)
    lo = int(math.floor(n * float(trim))) + 1
    hi = n + 1 - lo
    return float(np.mean(v[lo - 1:hi]))


def expected_magnitudes(counts, nb, ls, thr=1, trim=0.25):
    counts = np.asarray(counts)
    ls = np.asarray(ls, np.float64)
    N, C = counts.shape
    fpm = np.full((N, C), np.nan)
    nabove = np.zeros((N, C), np.int32)
    for i in range(C):
        oc = nb[i][nb[i] >= 0]
        sub = counts[:, oc]
        nabove[:, i] = (sub > thr).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = sub / ls[oc]  # (a library size of 0: Inf where valid, as in R)
        ok = sub >= thr
        for g in range(N):
            fpm[g, i] = trimmed_mean(val[g, ok[g]], trim)
    return fpm, nabove


# ------------------------------------------------------------------ model inputs
def r_median(v):
    v = np.sort(np.asarray(v, np.float64))
    n = len(v)
    if n == 0:
        return np.nan
    h = (n + 1) // 2
    return float(v[h - 1]) if n % 2 else float((v[h - 1] + v[h]) / 2)


def valid_genes(fpm, nabove, min_nonfailed=5, min_fpm=0):
    with np.errstate(invalid="ignore"):
        return (nabove >= min_nonfailed) & (fpm > min_fpm)


def fail_prior(counts, fpm, vi, thr=1):
    counts = np.asarray(counts)
    N, C = counts.shape
    out = np.full((N, C), np.nan)
    for i in range(C):
        g = np.flatnonzero(vi[:, i])
        low = counts[g, i] <= thr
        med = r_median(fpm[g, i][low])
        with np.errstate(invalid="ignore"):
            hit = low & (fpm[g, i] >= med)
        out[g, i] = np.where(hit, TP, 1 - TP)
    return out
