"""CPU tests of the optimal leaf ordering (include/scde_hip.h, "optimal leaf ordering"): the
numpy restatement of the contract (tests/olo_ref.py) against a brute force over all
orientations, the shape of its result, the numpy helper, and the argument checks the library
makes before it looks for a device."""
import numpy as np
import pytest

import olo_ref
from test_hclust import METHODS, ref_hclust

EPS = 2.0 ** -52


def _tree(n, method, seed=None):
    d = olo_ref.cluster_dist(n, seed)
    return d, ref_hclust(d, method)[0]


def _check_shape(merge, merge_out, order):
    """order is a permutation, every node's leaves are contiguous in it, the root is unflipped,
    and merge_out differs from merge only by column swaps."""
    n = merge.shape[0] + 1
    assert sorted(order.tolist()) == list(range(1, n + 1))
    same, swapped = (merge_out == merge).all(1), (merge_out == merge[:, ::-1]).all(1)
    assert (same | swapped).all()
    assert same[n - 2], "the root is never flipped"
    assert np.array_equal(order, olo_ref.leaves(merge_out))
    pos = np.empty(n + 1, np.int64)
    pos[order] = np.arange(n)
    members = {}
    for s in range(n - 1):
        mem = []
        for v in merge[s].tolist():
            mem += [-v] if v < 0 else members[v]
        members[s + 1] = mem
        p = pos[mem]
        assert p.max() - p.min() == len(mem) - 1, f"the leaves of step {s + 1} are not contiguous"


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", range(2, 11))
def test_restatement_is_optimal(n, method):
    d, merge = _tree(n, method)
    merge_out, order, length = olo_ref.order_optimal_ref(d, merge)
    best, _ = olo_ref.brute_force(d, merge)
    print(f"n={n} {method}: length {length!r}, brute force {best!r}, "
          f"input order {olo_ref.path_length(d, olo_ref.leaves(merge))!r}")
    assert abs(length - best) <= (n - 1) * EPS * length  # one rounding per addition
    _check_shape(merge, merge_out, order)
    assert length == olo_ref.path_length(d, order)
    if n == 2:
        assert np.array_equal(merge_out, merge)
    try:
        from scipy.cluster.hierarchy import leaves_list, linkage, optimal_leaf_ordering
        from scipy.spatial.distance import squareform
    except ImportError:
        return
    if method not in ("single", "complete", "average"):
        return  # (the names scipy shares)
    # scipy's result is one orientation of its own tree: the contract's order of that same tree
    # is no longer (an inequality only; scipy is never an equality oracle)
    y = squareform(d, checks=False)
    z = optimal_leaf_ordering(linkage(y, method), y)
    theirs = olo_ref.path_length(d, leaves_list(z) + 1)
    ours = olo_ref.order_optimal_ref(d, _scipy_merge(z))[2]
    assert ours <= theirs + n * EPS * ours


def _scipy_merge(z):
    """A scipy linkage as an R merge matrix (rows in scipy's step order)."""
    n = len(z) + 1
    enc = lambda v: -(int(v) + 1) if v < n else int(v) - n + 1  # noqa: E731
    return np.array([(enc(a), enc(b)) for a, b in z[:, :2]], np.int32)


@pytest.mark.parametrize("n", [17, 65])
def test_restatement_precisions_agree(n):
    """longdouble carries 11 more bits: where it picks another order, a choice hung on a rounding."""
    for method in ("ward.D", "single", "average"):
        d, merge = _tree(n, method)
        m64, o64, l64 = olo_ref.order_optimal_ref(d, merge)
        mld, old, lld = olo_ref.order_optimal_ref(d, merge, olo_ref.LD)
        _check_shape(merge, m64, o64)
        assert abs(l64 - float(lld)) <= (n - 1) * EPS * l64
        assert l64 <= olo_ref.path_length(d, olo_ref.leaves(merge))


def test_restatement_on_ties_and_special_trees():
    for n in (8, 9):
        d = olo_ref.tie_dist(n)
        merge = ref_hclust(d, "complete")[0]
        merge_out, order, length = olo_ref.order_optimal_ref(d, merge)
        assert length == olo_ref.brute_force(d, merge)[0]  # integer sums are exact
        _check_shape(merge, merge_out, order)
    d = olo_ref.line_dist(9)
    merge = ref_hclust(d, "single")[0]
    assert olo_ref.tree_plan(merge)["level"].max() == 8  # a caterpillar
    assert olo_ref.order_optimal_ref(d, merge)[2] == olo_ref.brute_force(d, merge)[0] == d[8, 0]
    merge = olo_ref.balanced_merge(8)
    assert olo_ref.tree_plan(merge)["level"].max() == 3
    d = olo_ref.cluster_dist(8, seed=5)
    _, _, length = olo_ref.order_optimal_ref(d, merge)
    assert abs(length - olo_ref.brute_force(d, merge)[0]) <= 7 * EPS * length


def test_restatement_1025_is_quick():
    import time
    d = olo_ref.cluster_dist(1025)
    merge = olo_ref.balanced_merge(1024)
    merge = np.vstack([merge, [[-1025, 1023]]]).astype(np.int32)
    t0 = time.perf_counter()
    merge_out, order, _ = olo_ref.order_optimal_ref(d, merge)
    print(f"n=1025 restatement: {time.perf_counter() - t0:.2f} s")
    _check_shape(merge, merge_out, order)


def test_leaf_order_length():
    from scde_amd import leaf_order_length
    d = np.zeros((4, 4))
    d[1, 0], d[2, 0], d[3, 0], d[2, 1], d[3, 1], d[3, 2] = 1.0, 2.0, 4.0, 8.0, 16.0, 32.0
    d[0, 1:] = np.nan  # the upper triangle is never read
    assert leaf_order_length(d, [1, 2, 3, 4]) == 1.0 + 8.0 + 32.0
    assert leaf_order_length(d, [3, 1, 4, 2]) == 2.0 + 4.0 + 16.0
    assert leaf_order_length(d, [2]) == 0.0
    big = np.zeros((4, 4))
    big[1, 0], big[2, 1], big[3, 2] = 1.0, 1e16, -1e16
    assert leaf_order_length(big, [1, 2, 3, 4]) == 0.0  # (1 + 1e16) - 1e16, left to right
    assert leaf_order_length(big, [4, 3, 2, 1]) == 1.0
    assert leaf_order_length(d, [1, 2, 3, 4]) == olo_ref.path_length(d, [1, 2, 3, 4])


def _call(f, d, ld, n, merge, merge_out=None, order=None):
    from scde_amd import _lib
    from scde_amd.api import _p
    merge = np.asfortranarray(merge, dtype=np.int32)
    merge_out = np.zeros((max(n - 1, 1), 2), np.int32, order="F") if merge_out is None else merge_out
    order = np.zeros(max(n, 1), np.int32) if order is None else order
    rc = f(None, _p(d), ld, n, _p(merge), _p(merge_out), _p(order), None)
    return rc, _lib.lib().scde_last_error().decode()


def test_earg_cases():
    """n < 2, ld < n, null and aliasing pointers, a merge matrix that is no tree, and a non-finite
    value of a host matrix are SCDE_EARG (1), checked before the device is looked for."""
    import scde_amd
    from scde_amd import _lib, cluster
    L = _lib.lib()
    d = np.asfortranarray(olo_ref.cluster_dist(5))
    good = np.array([[-1, -2], [-3, -4], [1, 2], [-5, 3]], np.int32)
    for f in (L.scde_order_optimal_host, L.scde_order_optimal_dev):
        rc, msg = _call(f, d, 5, 1, good)
        assert rc == 1 and "at least 2 objects" in msg
        rc, msg = _call(f, d, 4, 5, good)
        assert rc == 1 and "ld must be at least n" in msg
        m = np.asfortranarray(good)
        rc, msg = _call(f, d, 5, 5, m, merge_out=m)
        assert rc == 1 and "must not alias" in msg
        buf = np.zeros(13, np.int32)
        buf[:8] = m.ravel(order="F")
        other = np.zeros(8, np.int32)
        rc = f(None, d.ctypes.data, 5, 5, buf.ctypes.data, other.ctypes.data, buf[6:].ctypes.data, None)
        assert rc == 1 and b"must not alias" in L.scde_last_error()
        for bad, row, why in (
                ([[-1, -2], [-3, -1], [1, 2], [-5, 3]], 2, "observation that is used twice"),
                ([[-1, -2], [-3, 3], [2, -4], [-5, 1]], 2, "uses a step before it exists"),
                ([[-1, -2], [-3, 1], [1, -4], [-5, 3]], 3, "step that is used twice"),
                ([[-1, -2], [-3, 2], [1, -4], [-5, 3]], 2, "refers to its own step"),
                ([[-1, -2], [-3, -4], [1, 2], [-6, 3]], 4, "out of range"),
                ([[-1, -2], [-3, -4], [1, 0], [-5, 3]], 3, "out of range")):
            rc, msg = _call(f, d, 5, 5, np.array(bad, np.int32))
            assert rc == 1 and f"row {row}," in msg and why in msg, msg
        assert f(None, None, 5, 5, m.ctypes.data, m.ctypes.data, m.ctypes.data, None) == 1
        assert b"null" in L.scde_last_error()
    for v in (np.nan, np.inf, -np.inf):
        bad = d.copy(order="F")
        bad[3, 1] = v
        bad[4, 2] = v  # the first in column-major order is reported
        rc, msg = _call(L.scde_order_optimal_host, bad, 5, 5, good)
        assert rc == 1 and "non-finite distance at row 4, column 2" in msg
    with pytest.raises(ValueError, match="4 x 2"):
        cluster.order_optimal(cluster.HClust(good[:3], None, None, None), d)
    for f in ("order_optimal", "leaf_order_length"):
        assert getattr(scde_amd, f) is getattr(cluster, f)
