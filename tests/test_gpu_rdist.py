"""GPU tests of ``scde_amd.cluster.dist`` (csrc/rdist.hip) against the restatement in
tests/rdist_ref.py: equal bit for bit, for every method and for the host and the resident entry.

The kernel's pair tile is T = 64 objects and its column chunk K = 16; the shapes sit on both
sides of each, reach a second tile row and a third chunk, and are read with ld > n."""
import ctypes

import numpy as np
import pytest

import rdist_ref as R

pytestmark = pytest.mark.gpu

T, K = 64, 16
NS = (1, 2, 3, T - 1, T, T + 1, 2 * T + 1)
PS = (1, 2, K - 1, K, K + 1, 2 * K + 3)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, ref, what):
    assert got.shape == ref.shape, what
    bad = np.argwhere(bits(got) != bits(ref))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[0]}: {got[tuple(bad[0])]!r} " \
                          f"against {ref[tuple(bad[0])]!r}"


def nan_same(got, ref, what):
    """Bit equality, any NaN standing for any other (the payload of a NaN is not pinned)."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern"
    same(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(ref), 0.0, ref), what)


@pytest.fixture(scope="module")
def C():
    from scde_amd import cluster
    return cluster


def run_host(x, method, pad=0):
    """scde_dist_host on x stored with ld = n + pad (the padding rows hold NaN)."""
    from scde_amd import api
    from scde_amd._lib import check, lib
    n, p = x.shape
    buf = np.full((n + pad, p), np.nan, order="F")
    buf[:n] = x
    out = np.full((n, n), -1.0, order="F")
    check(lib().scde_dist_host(None, api._p(buf), n + pad, n, p, R.METHODS.index(method), api._p(out)))
    return out


def run_dev(x, method, pad=0):
    """scde_dist_dev on a resident x with ld = n + pad; the result read back."""
    from scde_amd import api
    from scde_amd._lib import check, lib
    L, ctx = lib(), api.default_context()
    n, p = x.shape
    buf = np.full((n + pad, p), np.nan, order="F")
    buf[:n] = x
    out = np.full((n, n), -1.0, order="F")
    xd, od = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, buf.nbytes, ctypes.byref(xd)))
    check(L.scde_dev_alloc(ctx.handle, out.nbytes, ctypes.byref(od)))
    try:
        check(L.scde_h2d(ctx.handle, xd, api._p(buf), buf.nbytes))
        check(L.scde_dist_dev(ctx.handle, xd, n + pad, n, p, R.METHODS.index(method), od))
        check(L.scde_d2h(ctx.handle, api._p(out), od, out.nbytes))
    finally:
        L.scde_dev_free(ctx.handle, xd)
        L.scde_dev_free(ctx.handle, od)
    return out


def data(n, p, seed=0):
    return np.random.default_rng(1000 * n + p + seed).normal(size=(n, p)) * 3.0


@pytest.mark.parametrize("method", R.METHODS)
def test_shapes_both_entries_bit_for_bit(method):
    for n in NS:
        for p in PS:
            x = data(n, p)
            ref = R.rdist(x, method)
            same(run_host(x, method, pad=3), ref, f"host {method} {n} x {p}")
            same(run_dev(x, method, pad=5), ref, f"dev {method} {n} x {p}")


@pytest.mark.parametrize("method", R.METHODS)
def test_python_entry_symmetry_diagonal_repeat(C, method):
    x = data(2 * T + 1, 2 * K + 3, seed=7)
    got = C.dist(x, method)
    same(got, R.rdist(x, method), method)
    same(got, got.T.copy(), f"{method}: symmetry")
    assert np.all(bits(np.diag(got)) == 0)
    same(C.dist(x, method), got, f"{method}: repeat")


def value_cases():
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(5)
    n, p = T + 7, 2 * K + 3
    base = rng.normal(size=(n, p))
    scattered = base.copy()
    scattered[rng.random((n, p)) < 0.15] = nan
    nocommon = base.copy()  # rows 0 and 1 share no column; row 2 is all NaN
    nocommon[0, ::2] = nan
    nocommon[1, 1::2] = nan
    nocommon[2] = nan
    infs = base.copy()
    infs[3, 4] = infs[5, 4] = inf  # Inf - Inf drops the column for the pair (3, 5)
    infs[6, 4] = -inf
    infs[7, :] = inf
    infs[8, :] = inf  # every column of the pair (7, 8) drops out
    onenan = base.copy()
    onenan[n - 1, p - 1] = nan
    zeros = base.copy()
    zeros[:, 0] = 0.0
    zeros[::2, 0] = -0.0
    zeros[:4] = 0.0
    zeros[1:3] = -0.0  # whole rows of zeros of either sign: distances +0
    return {"scattered NaN": scattered, "no common column": nocommon, "Inf": infs, "NaN-free": base,
            "one NaN": onenan, "signed zeros": zeros}


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("case", list(value_cases()))
def test_value_cases(C, method, case):
    x = value_cases()[case]
    ref = R.rdist(x, method)
    if case == "no common column":
        assert np.isnan(ref[1, 0]) and np.isnan(ref[2, 5])
    if case == "Inf":
        assert np.isnan(ref[8, 7]) and np.isinf(ref[6, 3]) and np.isfinite(ref[5, 3])
    for what, got in (("python", C.dist(x, method)), ("host", run_host(x, method, pad=1)),
                      ("dev", run_dev(x, method, pad=2))):
        nan_same(got, ref, f"{case}, {method}, {what}")
        nan_same(got, got.T.copy(), f"{case}, {method}, {what}: symmetry")
        assert np.all(bits(np.diag(got)) == 0)


def test_zero_columns_and_errors(C):
    got = C.dist(np.zeros((3, 0)))
    assert np.all(np.isnan(got[~np.eye(3, dtype=bool)])) and np.all(np.diag(got) == 0)
    with pytest.raises(ValueError):
        C.dist(np.zeros((3, 2)), "minkowski")
    from scde_amd import api
    from scde_amd._lib import lib
    x, out = np.zeros((3, 2), order="F"), np.zeros((3, 3), order="F")
    assert lib().scde_dist_host(None, api._p(x), 3, 3, 2, 3, api._p(out)) == 1  # SCDE_EARG
    assert lib().scde_dist_host(None, api._p(x), 2, 3, 2, 0, api._p(out)) == 1  # ld < n


@pytest.mark.parametrize("method", ["complete", "ward.D"])
def test_hclust_of_dist_resident_chain(C, method):
    x = data(T + 9, K + 5, seed=3)
    hc = C.hclust_dist(x, "euclidean", method)
    ref = C.hclust(R.rdist(x, "euclidean"), method)
    assert np.array_equal(hc.merge, ref.merge) and np.array_equal(hc.order, ref.order)
    assert np.array_equal(bits(hc.height), bits(ref.height))
