"""The optimal-leaf-ordering contract of include/scde_hip.h restated literally in numpy (float64
and np.longdouble), a brute force over all 2^(n - 1) orientations, and the inputs the tests of
tests/test_olo.py and tests/test_gpu_olo.py share.  Not a test module."""
import itertools

import numpy as np

LD = np.longdouble


# ------------------------------------------------------------------ inputs
def cluster_points(n, seed=None, dim=5, k=4):
    """n points around k Gaussian cluster centres."""
    rng = np.random.default_rng(9000 + n if seed is None else seed)
    centres = rng.normal(0, 4, (k, dim))
    return centres[rng.integers(0, k, n)] + rng.normal(0, 1, (n, dim))


def euclid(x):
    """Symmetric Euclidean distance matrix, zero diagonal."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if x.shape[0] == 1:
        x = x.T
    g = x[:, None, :] - x[None, :, :]
    d = np.sqrt((g * g).sum(-1))
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def cluster_dist(n, seed=None):
    return euclid(cluster_points(n, seed))


def line_dist(n):
    """Points on a line with growing gaps: single linkage gives a caterpillar of depth n - 1."""
    return euclid(np.cumsum(1.02 ** np.arange(n)))


def tie_dist(n):
    """Integer distances from {1, 2, 3}: many orientations are optimal and every sum is exact."""
    rng = np.random.default_rng(300 + n)
    d = np.tril(rng.integers(1, 4, (n, n)).astype(np.float64), -1)
    return d + d.T


def balanced_merge(n):
    """A perfectly balanced merge matrix over n = 2^k observations."""
    assert n >= 2 and n & (n - 1) == 0
    rows, cur = [], [-(i + 1) for i in range(n)]
    while len(cur) > 1:
        nxt = []
        for i in range(0, len(cur), 2):
            rows.append((cur[i], cur[i + 1]))
            nxt.append(len(rows))
        cur = nxt
    return np.array(rows, np.int32)


# ------------------------------------------------------------------ the tree
def tree_plan(merge):
    """Per step (0-based) the position intervals: lo, mid, hi, the children's splits lmid / rmid
    (-1: a leaf), the children's steps left / right (-1: a leaf), the level; and perm (position
    -> 0-based observation), the input tree's own left-to-right leaf order."""
    merge = np.asarray(merge)
    m = merge.shape[0]
    n = m + 1
    size, level = np.zeros(m, np.int64), np.zeros(m, np.int64)
    for s in range(m):
        for v in merge[s].tolist():
            size[s] += 1 if v < 0 else size[v - 1]
            level[s] = max(level[s], 1 if v < 0 else level[v - 1] + 1)
    lo, mid, hi = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    perm = np.zeros(n, np.int64)
    for s in range(m - 1, -1, -1):
        l, r = int(merge[s, 0]), int(merge[s, 1])
        mid[s] = lo[s] + (1 if l < 0 else size[l - 1])
        hi[s] = lo[s] + size[s]
        if l < 0:
            perm[lo[s]] = -l - 1
        else:
            lo[l - 1] = lo[s]
        if r < 0:
            perm[mid[s]] = -r - 1
        else:
            lo[r - 1] = mid[s]
    left = np.where(merge[:, 0] < 0, -1, merge[:, 0] - 1)
    right = np.where(merge[:, 1] < 0, -1, merge[:, 1] - 1)
    lmid = np.where(left < 0, -1, mid[np.maximum(left, 0)])
    rmid = np.where(right < 0, -1, mid[np.maximum(right, 0)])
    return dict(n=n, lo=lo, mid=mid, hi=hi, lmid=lmid, rmid=rmid, left=left, right=right, level=level, perm=perm)


def leaves(merge):
    """1-based leaves of a merge matrix left to right, column 1 as the left child."""
    merge = np.asarray(merge)
    out, stack = [], [merge.shape[0]]
    while stack:
        v = stack.pop()
        if v < 0:
            out.append(-v)
        else:
            stack.extend([int(merge[v - 1, 1]), int(merge[v - 1, 0])])
    return np.array(out, np.int32)


def path_length(d, order, T=np.float64):
    """d (lower triangle) summed along the 1-based order, left to right, in T."""
    o = np.asarray(order, np.int64) - 1
    total = T(0)
    for v in np.asarray(d)[np.maximum(o[:-1], o[1:]), np.minimum(o[:-1], o[1:])].tolist():
        total = total + T(v)
    return total


# ------------------------------------------------------------------ the contract
def _minplus(a, b, budget=1 << 22):
    """min over i of a[r, i] + b[i, c], rows in chunks so that the temporary stays small."""
    out = np.empty((a.shape[0], b.shape[1]), a.dtype)
    step = max(1, budget // max(1, a.shape[1] * b.shape[1]))
    for r in range(0, a.shape[0], step):
        out[r:r + step] = (a[r:r + step, :, None] + b[None, :, :]).min(axis=1)
    return out


def table(d, merge, T=np.float64):
    """(M, D, plan): the table of the contract and d in leaf-position order, in T."""
    p = tree_plan(merge)
    n, perm = p["n"], p["perm"]
    low = np.tril(np.asarray(d, dtype=np.float64), -1)
    D = (low + low.T)[np.ix_(perm, perm)].astype(T)
    M = np.zeros((n, n), T)
    for s in range(n - 1):  # a step's children are earlier steps
        lo, mid, hi, lmid, rmid = (int(p[k][s]) for k in ("lo", "mid", "hi", "lmid", "rmid"))
        # 1. T(u, k) = min_m fl(M(u, m) + d(m, k)), m in far(L, u)
        if lmid < 0:
            t = M[lo:mid, lo:mid] + D[lo:mid, mid:hi]
        else:
            t = np.vstack([_minplus(M[lo:lmid, lmid:mid], D[lmid:mid, mid:hi]),
                           _minplus(M[lmid:mid, lo:lmid], D[lo:lmid, mid:hi])])
        # 2. M(u, w) = min_k fl(T(u, k) + M(k, w)), k in far(R, w)
        if rmid < 0:
            b = t + M[mid:hi, mid:hi]
        else:
            c = rmid - mid
            b = np.hstack([_minplus(t[:, c:], M[rmid:hi, mid:rmid]), _minplus(t[:, :c], M[mid:rmid, rmid:hi])])
        M[lo:mid, mid:hi] = b
        M[mid:hi, lo:mid] = b.T
    return M, D, p


def order_optimal_ref(d, merge, T=np.float64):
    """(merge_out, order_out, length) of the contract, all arithmetic in T."""
    merge = np.asarray(merge)
    M, D, p = table(d, merge, T)
    n = p["n"]
    root = n - 2
    ex, ey = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    flip = np.zeros(n - 1, bool)
    lo, mid, hi = int(p["lo"][root]), int(p["mid"][root]), int(p["hi"][root])
    blk = M[lo:mid, mid:hi]
    u, w = divmod(int(np.argmin(blk)), hi - mid)  # the first minimum in (p(u), p(w)) order
    ex[root], ey[root] = lo + u, mid + w
    for s in range(root, -1, -1):  # a parent's step is larger than its children's
        lo, mid, hi, lmid, rmid = (int(p[k][s]) for k in ("lo", "mid", "hi", "lmid", "rmid"))
        x, y = int(ex[s]), int(ey[s])
        flip[s] = x >= mid
        a, b = (y, x) if flip[s] else (x, y)
        assert lo <= a < mid <= b < hi
        m0, m1 = (a, a + 1) if lmid < 0 else (lmid, mid) if a < lmid else (lo, lmid)
        k0, k1 = (b, b + 1) if rmid < 0 else (rmid, hi) if b < rmid else (mid, rmid)
        cost = (M[a, m0:m1][:, None] + D[m0:m1, k0:k1]) + M[k0:k1, b][None, :]
        mi, ki = divmod(int(np.argmin(cost)), k1 - k0)  # the first minimum in (p(m), p(k)) order
        assert cost[mi, ki] == M[a, b], "the forward form's minimum is the table entry, bit for bit"
        m, k = m0 + mi, k0 + ki
        if p["left"][s] >= 0:
            ex[p["left"][s]], ey[p["left"][s]] = (m, a) if flip[s] else (a, m)
        if p["right"][s] >= 0:
            ex[p["right"][s]], ey[p["right"][s]] = (b, k) if flip[s] else (k, b)
    merge_out = np.where(flip[:, None], merge[:, ::-1], merge).astype(np.int32)
    order = leaves(merge_out)
    return merge_out, order, path_length(d, order, T)


def brute_force(d, merge, T=np.float64):
    """The smallest path length over all 2^(n - 1) orientations, and one order that has it."""
    merge = np.asarray(merge)
    best, best_order = None, None
    for bits in itertools.product((False, True), repeat=merge.shape[0]):
        order = leaves(np.where(np.array(bits)[:, None], merge[:, ::-1], merge))
        length = path_length(d, order, T)
        if best is None or length < best:
            best, best_order = length, order
    return best, best_order
