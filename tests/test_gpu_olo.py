"""GPU tests of the optimal leaf ordering (csrc/olo.hip): merge_out, order_out and length equal
the float64 restatement of the contract (tests/olo_ref.py) -- the same IEEE operations, and min
is exact, so equality is unconditional -- at the tile edges of the kernels (64 x 64 output tiles,
16 inner indices per stage, 8 x 8 per lane), on deep and balanced trees, on ties, through both
entry points and through pagoda_cluster_cells; and the error paths."""
import ctypes

import numpy as np
import pytest

import olo_ref
from test_hclust import METHODS, _cells_varinfo, _dev_free, _dev_put

pytestmark = pytest.mark.gpu

# 2..4: the smallest trees; 15..17: the inner stage; 63..65, 127..129: one and two output tiles;
# 257: five tiles with a remainder of one
SIZES = [2, 3, 4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
_REF = {}


def _ref(key, d, merge):
    """The restatement of a case, computed once."""
    if key not in _REF:
        _REF[key] = olo_ref.order_optimal_ref(d, merge)
    return _REF[key]


def _assert_equal(got, length, ref, d, what):
    merge_out, order, ref_length = ref
    print(f"{what}: length {length!r}, restatement {ref_length!r}, "
          f"input order {olo_ref.path_length(d, olo_ref.leaves(got.merge_in))!r}")
    assert np.array_equal(got.merge, merge_out), f"{what}: merge_out differs"
    assert np.array_equal(got.order, order), f"{what}: order_out differs"
    assert length == ref_length, f"{what}: length {length!r} != {ref_length!r}"


def _run(d, merge, what, key=None):
    from scde_amd import order_optimal
    from scde_amd.cluster import HClust
    hc = HClust(np.asarray(merge), None, None, "x", ["a"])
    got, length = order_optimal(hc, d, return_length=True)
    got.merge_in = hc.merge
    assert got.method == "x" and got.labels == ["a"] and got.height is None
    _assert_equal(got, length, _ref(key or what, d, hc.merge), d, what)
    return got, length


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", METHODS)
def test_equals_restatement(method, n):
    from scde_amd import hclust, leaf_order_length
    d = olo_ref.cluster_dist(n)
    hc = hclust(d, method=method)
    got, length = _run(d, hc.merge, f"{method} n={n}")
    assert length == leaf_order_length(d, got.order)
    assert length <= leaf_order_length(d, hc.order) * (1 + n * 2.0 ** -52)
    if n == 2:
        assert np.array_equal(got.merge, hc.merge) and np.array_equal(got.order, hc.order)


@pytest.mark.parametrize("method", ["ward.D", "single"])
def test_equals_restatement_1025(method):
    from scde_amd import hclust
    d = olo_ref.cluster_dist(1025)
    _run(d, hclust(d, method=method).merge, f"{method} n=1025")


@pytest.mark.parametrize("n", [65, 257])
def test_caterpillar(n):
    from scde_amd import hclust
    d = olo_ref.line_dist(n)
    hc = hclust(d, method="single")
    assert olo_ref.tree_plan(hc.merge)["level"].max() == n - 1
    _, length = _run(d, hc.merge, f"caterpillar n={n}")
    # the line itself, from either end (the root is not flipped, so the end is the tree's): the
    # same n - 1 gaps added in another order, one rounding per addition
    line = olo_ref.path_length(d, np.arange(1, n + 1))
    assert abs(length - line) <= (n - 1) * 2.0 ** -52 * line


def test_balanced():
    merge = olo_ref.balanced_merge(256)
    assert olo_ref.tree_plan(merge)["level"].max() == 8
    _run(olo_ref.cluster_dist(256), merge, "balanced n=256")


@pytest.mark.parametrize("n", [64, 65])
def test_ties(n):
    from scde_amd import hclust
    d = olo_ref.tie_dist(n)
    _run(d, hclust(d, method="complete").merge, f"ties n={n}")


def _c_entry(a, ld, n, merge, dev):
    """scde_order_optimal_host / _dev on the buffer a (ld x n, column-major): (rc, message,
    merge_out, order, length, the buffer afterwards)."""
    from scde_amd import _lib, api
    L, ctx = _lib.lib(), api.default_context()
    merge = np.asfortranarray(merge, dtype=np.int32)
    merge_out, order = np.zeros((n - 1, 2), np.int32, order="F"), np.zeros(n, np.int32)
    length = ctypes.c_double(-1.0)
    after = None
    if dev:
        p = _dev_put(a)
        try:
            rc = L.scde_order_optimal_dev(ctx.handle, p, ld, n, api._p(merge), api._p(merge_out), api._p(order),
                                          ctypes.byref(length))
            msg = L.scde_last_error().decode()
            after = np.empty_like(a)
            _lib.check(L.scde_d2h(ctx.handle, api._p(after), p, a.nbytes))
        finally:
            _dev_free(p)
    else:
        rc = L.scde_order_optimal_host(ctx.handle, api._p(a), ld, n, api._p(merge), api._p(merge_out), api._p(order),
                                       ctypes.byref(length))
        msg = L.scde_last_error().decode()
    return rc, msg, merge_out, order, length.value, after


@pytest.mark.parametrize("n", [65, 129])
def test_dev_equals_host_and_only_the_lower_triangle_is_read(n):
    """_dev on a resident matrix gives _host's result and leaves the matrix alone; with ld > n and
    NaN in the padding, on the diagonal and above it, nothing changes."""
    from scde_amd import hclust
    d = olo_ref.cluster_dist(n)
    merge = hclust(d, method="average").merge
    ref = _ref(f"average n={n}", d, merge)
    ld = n + 3
    padded = np.full((ld, n), np.nan, order="F")
    padded[:n][np.tril_indices(n, -1)] = d[np.tril_indices(n, -1)]
    for a, lda in ((np.asfortranarray(d), n), (padded, ld)):
        for dev in (False, True):
            rc, msg, merge_out, order, length, after = _c_entry(a, lda, n, merge, dev)
            assert rc == 0, msg
            assert np.array_equal(merge_out, ref[0]) and np.array_equal(order, ref[1]) and length == ref[2]
            if dev:
                assert np.array_equal(after, a, equal_nan=True)


def test_pagoda_cluster_cells_optimal_order():
    from scde_amd import hclust, leaf_order_length, order_optimal, pagoda_cluster_cells
    tam, vi = _cells_varinfo()
    for method in ("ward.D", "complete"):
        plain = pagoda_cluster_cells(tam, vi, method=method, return_details=True)
        dm = plain["distance"]
        res = pagoda_cluster_cells(tam, vi, method=method, return_details=True, optimal_order=True)
        assert np.array_equal(res["distance"], dm) and res["genes"] == plain["genes"]
        hc = hclust(dm, method=method)
        want, length = order_optimal(hc, dm, return_length=True)
        got = res["clustering"]
        assert np.array_equal(got.merge, want.merge) and np.array_equal(got.order, want.order)
        assert np.array_equal(got.height, hc.height) and got.labels == vi["cells"] and got.method == method
        ref = olo_ref.order_optimal_ref(dm, hc.merge)
        assert np.array_equal(got.merge, ref[0]) and np.array_equal(got.order, ref[1]) and length == ref[2]
        assert leaf_order_length(dm, got.order) == length <= leaf_order_length(dm, hc.order)
        # the default is the tree as it was
        off = pagoda_cluster_cells(tam, vi, method=method, optimal_order=False)
        for t in (off, plain["clustering"]):
            assert np.array_equal(t.merge, hc.merge) and np.array_equal(t.order, hc.order)
            assert np.array_equal(t.height, hc.height)


def test_errors():
    from scde_amd import ScdeError, _lib, hclust, order_optimal
    from scde_amd.cluster import HClust
    n = 20
    d = olo_ref.cluster_dist(n)
    hc = hclust(d, method="average")
    for v in (np.nan, np.inf, -np.inf):
        bad = np.asfortranarray(d.copy())
        bad[7, 3] = v
        bad[9, 5] = v
        bad[3, 7] = 0.0
        for dev in (False, True):
            rc, msg, *_ = _c_entry(bad, n, n, hc.merge, dev)
            assert rc == 1 and "non-finite distance at row 8, column 4 (1-based)" in msg, msg
        with pytest.raises(ScdeError, match="non-finite distance at row 8, column 4"):
            order_optimal(hc, bad)
    for edit, text in ((lambda m: m.__setitem__((5, 0), m[0, 0]), "observation that is used twice"),
                       (lambda m: m.__setitem__((2, 1), 19), "uses a step before it exists"),
                       (lambda m: m.__setitem__((n - 2, 0), m[n - 2, 1]), "step that is used twice")):
        merge = hc.merge.copy()
        edit(merge)
        with pytest.raises(ScdeError, match=text):
            order_optimal(HClust(merge, None, None, None), d)
    L = _lib.lib()
    a = np.asfortranarray(d)
    m = np.asfortranarray(hc.merge)
    order = np.zeros(n, np.int32)
    for f in (L.scde_order_optimal_host, L.scde_order_optimal_dev):
        assert f(None, a.ctypes.data, n, 1, m.ctypes.data, np.zeros(2, np.int32).ctypes.data, order.ctypes.data,
                 None) == 1
        assert b"at least 2 objects are needed (n = 1)" in L.scde_last_error()
        assert f(None, a.ctypes.data, n, n, m.ctypes.data, m.ctypes.data, order.ctypes.data, None) == 1
        assert b"must not alias" in L.scde_last_error()
    with pytest.raises(ValueError, match="at least 2"):
        order_optimal(hc, np.zeros((1, 1)))
    # a failed call leaves the context usable
    got = order_optimal(hc, d)
    assert np.array_equal(got.order, olo_ref.order_optimal_ref(d, hc.merge)[1])
