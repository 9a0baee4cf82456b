"""The Spearman contract of include/scde_hip.h restated in numpy and Python integers: the rank
transform, the pairwise-complete cell similarity and the gene-cluster distance.  No GPU, and
nothing of the package under test."""
import math

import numpy as np

from knn_ref import average_rank


def rank(v):
    """R's rank(v, ties.method = "average", na.last = "keep"): a NaN stays NaN, the other values
    are ranked among themselves (-0.0 == 0.0 in numpy as in R, so they tie)."""
    v = np.asarray(v, np.float64)
    out = np.full(v.shape, np.nan)
    ok = ~np.isnan(v)
    out[ok] = average_rank(v[ok])
    out[~ok] = v[~ok]
    return out


def rank_columns(x):
    x = np.asarray(x, np.float64)
    return np.column_stack([rank(x[:, j]) for j in range(x.shape[1])]).reshape(x.shape)


def doubled_ranks(c):
    """a_g = 2 #{h : c_h < c_g} + #{h : c_h = c_g} + 1 of an integer vector, as Python integers."""
    vals, inv, cnt = np.unique(np.asarray(c), return_inverse=True, return_counts=True)
    below = np.cumsum(cnt) - cnt
    return [2 * int(below[k]) + int(cnt[k]) + 1 for k in inv.reshape(-1)]


def common_genes(ci, cj, thr):
    return np.flatnonzero((np.asarray(ci) >= thr) & (np.asarray(cj) >= thr))


def pair_similarity(ci, cj, thr=1):
    """The contract, literally: integer centred sums, then three correctly rounded operations."""
    s = common_genes(ci, cj, thr)
    m = len(s)
    if m == 0:
        return math.nan
    a, b = doubled_ranks(np.asarray(ci)[s]), doubled_ranks(np.asarray(cj)[s])
    assert sum(a) == sum(b) == m * (m + 1)
    mm = m * (m + 1) ** 2
    sab = sum(x * y for x, y in zip(a, b)) - mm
    saa = sum(x * x for x in a) - mm
    sbb = sum(y * y for y in b) - mm
    if saa == 0 or sbb == 0:
        return math.nan
    r = float(sab) / math.sqrt(float(saa) * float(sbb))
    return max(-1.0, min(1.0, r))


def cell_similarity(counts, thr=1):
    counts = np.asarray(counts)
    C = counts.shape[1]
    out = np.full((C, C), np.nan)
    for i in range(C):
        for j in range(i, C):
            out[i, j] = out[j, i] = pair_similarity(counts[:, i], counts[:, j], thr)
    return out


def gene_distance(mat):
    """1 - cor(t(mat), method = "spearman") of a genes x cells matrix."""
    return 1 - np.corrcoef(np.vstack([rank(row) for row in np.asarray(mat, np.float64)]))
