"""Hierarchical clustering (scde_amd/cluster.py, csrc/hclust.hip; contract in include/scde_hip.h).

The reference of every comparison is ``ref_hclust`` below: the header's contract evaluated
literally in numpy -- a matrix with inf outside the active upper triangle, ``np.argmin`` of the
flat row-major matrix (the lexicographic (d, i, j) minimum), the update formulas in the written
order -- in float64 and in np.longdouble.  The GPU's merges, heights and order must EQUAL the
float64 restatement's (array_equal): the kernel performs the same IEEE operations in the same
order with contraction off.  A case is usable for that only if no decision in it hangs on a
rounding, which the CPU tests establish: the float64 and longdouble merge sequences of every
tie-free case the GPU tests use are identical.  The tie cases use small integers: single and
complete are exact on them; average is held to the float64 evaluation operation for operation.

The restatement is cross-checked against scipy where scipy is present (same cluster sets;
single / complete heights equal; the others within 64 x the restatement's own float64 -
longdouble difference).  That R picks the same pair on tied distances is read from R's
algorithm; no R was run.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden, gpu_available

LD = np.longdouble
METHODS = ["ward.D", "ward.D2", "single", "complete", "average", "mcquitty"]
SIZES = [2, 3, 63, 64, 65, 257, 1025]  # the wave edges and one past a 1024-thread block's single pass


# ------------------------------------------------------------------ the restatement
def ref_steps(d, method, T=np.float64):
    """The raw steps [(i, j, h)] (0-based slots, i < j) of the header's contract."""
    d = np.asarray(d)
    n = d.shape[0]
    a = np.full((n, n), np.inf, dtype=T)
    iu = np.triu_indices(n, 1)
    a[iu] = d.T[iu].astype(T)  # a[i, j] = d(j, i), the strict lower triangle
    if method == "ward.D2":
        a[iu] = a[iu] * a[iu]
    size = np.ones(n, dtype=T)
    active = np.ones(n, bool)
    steps = []
    for _ in range(n - 1):
        i, j = divmod(int(np.argmin(a)), n)
        h = a[i, j]
        steps.append((i, j, h))
        active[j] = False
        ks = np.nonzero(active)[0]
        ks = ks[ks != i]
        lo_i, hi_i = np.minimum(ks, i), np.maximum(ks, i)
        lo_j, hi_j = np.minimum(ks, j), np.maximum(ks, j)
        dik, djk = a[lo_i, hi_i], a[lo_j, hi_j]
        ni, nj, nk = size[i], size[j], size[ks]
        if method in ("ward.D", "ward.D2"):
            new = ((ni + nk) * dik + (nj + nk) * djk - nk * h) / (ni + nj + nk)
        elif method == "single":
            new = np.minimum(dik, djk)
        elif method == "complete":
            new = np.maximum(dik, djk)
        elif method == "average":
            new = (ni * dik + nj * djk) / (ni + nj)
        elif method == "mcquitty":
            new = (dik + djk) / 2
        else:
            raise ValueError(method)
        a[lo_i, hi_i] = new
        a[j, :] = np.inf
        a[:, j] = np.inf
        size[i] = ni + nj
    return steps


def r_encode(n, steps, method):
    """R's merge ((n - 1) x 2), height and order (1-based) from the raw steps."""
    label = [-(k + 1) for k in range(n)]
    merge = np.zeros((n - 1, 2), np.int32)
    for s, (i, j, _) in enumerate(steps):
        a, b = label[i], label[j]
        if a < 0 and b < 0:
            row = (a, b)           # two singletons: increasing index (i < j)
        elif a < 0 or b < 0:
            row = (min(a, b), max(a, b))  # the singleton first
        else:
            row = (min(a, b), max(a, b))  # two clusters: increasing step
        merge[s] = row
        label[i] = s + 1
    hs = np.array([h for _, _, h in steps])
    height = (np.sqrt(hs) if method == "ward.D2" else hs)

    def leaves(v):
        out, stack = [], [v]
        while stack:
            v = stack.pop()
            if v < 0:
                out.append(-v)
            else:
                stack.extend([merge[v - 1, 1], merge[v - 1, 0]])
        return out
    return merge, height, np.array(leaves(n - 1), np.int32)


def ref_hclust(d, method, T=np.float64):
    n = np.asarray(d).shape[0]
    return r_encode(n, ref_steps(d, method, T), method)


class Tree:
    def __init__(self, merge, height):
        self.merge, self.height = merge, height


_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def corr_dist(n, p=12, seed=None):
    """1 - correlation of n random p-vectors, symmetric, zero diagonal: tie-free."""
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    d = 1 - np.corrcoef(rng.standard_normal((n, p)))
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return d


def tie_dist(n):
    rng = np.random.default_rng(n)
    d = np.tril(rng.integers(1, 5, (n, n)).astype(np.float64), -1)
    return d + d.T


def _ref(kind, n, method, T=np.float64):
    d = {"corr": corr_dist, "tie": tie_dist, "corr8": lambda n: corr_dist(n, 8)}[kind](n)
    return _cached((kind, n, method, T), lambda: ref_hclust(d, method, T))


def ref_checked(d, method):
    """The float64 restatement of a matrix made at run time, after checking what the fixed cases
    get checked on the CPU: longdouble picks the same pairs."""
    ref = ref_hclust(d, method)
    assert np.array_equal(ref[0], ref_hclust(d, method, LD)[0]), "a merge of this case hangs on a rounding"
    return ref


def assert_same_tree(got, ref, what):
    merge, height, order = ref
    assert np.array_equal(got.merge, merge), f"{what}: merge differs"
    assert np.array_equal(got.order, order), f"{what}: order differs"
    err = float(np.max(np.abs(got.height - height), initial=0.0))
    print(f"{what}: max |height - restatement| {err:.3e}")
    assert np.array_equal(got.height, height), f"{what}: heights differ by up to {err:.3e}"


# the tie-free cases of the GPU tests: (kind, n, method)
def _gpu_cases():
    out = [("corr", n, m) for m in METHODS for n in SIZES]
    out += [("corr8", 1500, m) for m in ("ward.D", "complete")]
    out += [("corr", 300, m) for m in ("ward.D", "mcquitty")]  # the batch test's extra size
    return out


def _sets(n, z):
    """The member sets of a scipy linkage's steps (ids >= n name earlier steps)."""
    members = {k: frozenset([k]) for k in range(n)}
    for s, row in enumerate(z):
        members[n + s] = members[int(row[0])] | members[int(row[1])]
    return {members[n + s] for s in range(len(z))}


def _restatement_sets(n, steps):
    slot = {k: frozenset([k]) for k in range(n)}
    out = set()
    for i, j, _ in steps:
        slot[i] = slot[i] | slot[j]
        out.add(slot[i])
    return out


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("method", METHODS)
def test_restatement_against_scipy(method):
    H = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    for n in (2, 3, 65, 300):
        if n == 2 and method == "ward.D":
            continue  # scipy's route there is sqrt then square of one value: a rounding of its own, nothing of ours
        rng = np.random.default_rng(7)
        d = 1 - np.corrcoef(rng.standard_normal((n, 12)))
        d = (d + d.T) / 2
        np.fill_diagonal(d, 0.0)
        s64, sld = ref_steps(d, method, np.float64), ref_steps(d, method, LD)
        assert [(i, j) for i, j, _ in s64] == [(i, j) for i, j, _ in sld], (method, n)
        h64 = np.array([h for _, _, h in s64])
        hld = np.array([h for _, _, h in sld])
        y = squareform(d, checks=False)
        if method == "ward.D":     # scipy's ward on sqrt(d), heights squared
            hs = H.linkage(np.sqrt(y), "ward")
            zh = hs[:, 2] ** 2
        elif method == "ward.D2":
            hs = H.linkage(y, "ward")
            zh = hs[:, 2]
            h64, hld = np.sqrt(h64), np.sqrt(hld)
        else:
            hs = H.linkage(y, {"mcquitty": "weighted"}.get(method, method))
            zh = hs[:, 2]
        assert _sets(n, hs) == _restatement_sets(n, s64), (method, n)
        if method in ("single", "complete"):
            assert np.array_equal(zh, h64), (method, n)
        else:
            own = float(np.max(np.abs(h64 - hld)))
            err = float(np.max(np.abs(zh - hld)))
            print(f"{method} n={n}: scipy max err {err:.3e}, restatement's own {own:.3e}")
            assert err <= 64 * own, (method, n, err, own)


@pytest.mark.parametrize("kind,n,method", _gpu_cases())
def test_restatement_precisions_agree(kind, n, method):
    """The precondition of the GPU tests' equality: no merge of a tie-free case hangs on a
    rounding (float64 and longdouble pick the same pairs in the same order)."""
    m64, h64, o64 = _ref(kind, n, method)
    mld, hld, old = _ref(kind, n, method, LD)
    assert np.array_equal(m64, mld) and np.array_equal(o64, old)
    assert np.max(np.abs(h64 - hld)) <= 1e-9 * max(1.0, float(np.max(np.abs(h64))))
    assert np.all(np.diff(h64) >= 0)  # these linkages are monotone


@pytest.mark.parametrize("method", ["single", "complete", "average"])
def test_restatement_on_ties(method):
    """The tie cases do have tied minima.  single and complete only move values, so they are
    exact in any precision; average's quotients by 3, 5, ... round, so an exact tie may be one
    in float64 and not in longdouble: there the GPU is held to the float64 evaluation alone,
    operation for operation."""
    for n in (40, 130):
        m64, h64, o64 = _ref("tie", n, method)
        if method != "average":
            mld, hld, old = _ref("tie", n, method, LD)
            assert np.array_equal(m64, mld) and np.array_equal(o64, old) and np.array_equal(h64, hld)
        assert len(set(h64.tolist())) < len(h64)  # tied heights do occur
        assert np.all(np.diff(h64) >= 0)


def test_restatement_precisions_agree_batch_of_300():
    for p in range(300):
        d = corr_dist(33, seed=100 + p)
        assert np.array_equal(ref_hclust(d, "ward.D")[0], ref_hclust(d, "ward.D", LD)[0]), p


def _first_appearance(lab):
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    rank = np.empty(len(first), int)
    rank[np.argsort(first)] = np.arange(1, len(first) + 1)
    return rank[np.ravel(inv)]


def test_cutree():
    from scde_amd.cluster import cutree
    n = 65
    d = corr_dist(n)
    for method in ("ward.D", "average"):
        merge, height, _ = _ref("corr", n, method)
        hc = Tree(merge, height)
        for k in (1, n):
            lab = cutree(hc, k=k)
            assert np.array_equal(lab, np.ones(n) if k == 1 else np.arange(1, n + 1))
        below, above = height[0] / 2, height[-1] * 2
        assert np.array_equal(cutree(hc, h=below), np.arange(1, n + 1))
        assert np.array_equal(cutree(hc, h=above), np.ones(n))
        # a cut at a height includes that step (<=)
        assert np.array_equal(cutree(hc, h=height[9]), cutree(hc, k=n - 10))
        assert np.array_equal(cutree(hc, h=np.nextafter(height[9], -np.inf)), cutree(hc, k=n - 9))
        for bad in (dict(), dict(k=3, h=1.0)):
            with pytest.raises(ValueError, match="exactly one"):
                cutree(hc, **bad)
        for k in (0, n + 1):
            with pytest.raises(ValueError, match="k must be"):
                cutree(hc, k=k)
        with pytest.raises(ValueError, match="monotone"):
            cutree(Tree(merge, height[::-1].copy()), h=1.0)
    H = pytest.importorskip("scipy.cluster.hierarchy")
    from scipy.spatial.distance import squareform
    for method, sm in (("average", "average"), ("complete", "complete"), ("mcquitty", "weighted")):
        merge, height, _ = _ref("corr", n, method)
        z = H.linkage(squareform(d, checks=False), sm)
        for k in (2, 3, 7, 20, 64):
            want = _first_appearance(H.cut_tree(z, n_clusters=k)[:, 0])
            got = cutree(Tree(merge, height), k=k)
            assert np.array_equal(got, want), (method, k)
            assert got[0] == 1 and np.array_equal(got, _first_appearance(got))


def _five():
    """Objects 1..5, complete linkage.
    d(2,5) = 1                      step 1: -2 -5            (slots 1, 4 -> slot 1)
    d(1,3) = 2                      step 2: -1 -3            (slots 0, 2 -> slot 0)
    d(4,2) = 3, d(4,5) = 3.5        step 3: 4 joins {2,5} at max = 3.5: a singleton before a
                                    cluster: -4 1            (slots 1, 3; {1,3}-4 is max(6, 7))
    d(1,2) = 8, d(1,5) = 9, d(3,2) = 8.5, d(3,5) = 10, d(4,1) = 6, d(4,3) = 7
                                    step 4: {1,3} (step 2) and {4,2,5} (step 3) at 10: 2 3
    order: step 4 -> left step 2 -> 1 3; right step 3 -> 4, then step 1 -> 2 5."""
    d = np.zeros((5, 5))
    for (a, b), v in {(2, 5): 1, (1, 3): 2, (4, 2): 3, (4, 5): 3.5, (1, 2): 8, (1, 5): 9, (3, 2): 8.5, (3, 5): 10,
                      (4, 1): 6, (4, 3): 7}.items():
        d[a - 1, b - 1] = d[b - 1, a - 1] = v
    merge = np.array([[-2, -5], [-1, -3], [-4, 1], [2, 3]], np.int32)
    return d, merge, np.array([1, 2, 3.5, 10]), np.array([1, 3, 4, 2, 5], np.int32)


def test_r_encoding_worked_example():
    from scde_amd.cluster import cutree
    d, merge, height, order = _five()
    steps = ref_steps(d, "complete")
    assert [(i, j) for i, j, _ in steps] == [(1, 4), (0, 2), (1, 3), (0, 1)]
    m, h, o = r_encode(5, steps, "complete")
    assert np.array_equal(m, merge) and np.array_equal(h, height) and np.array_equal(o, order)
    assert np.array_equal(cutree(Tree(merge, height), k=2), [1, 2, 1, 2, 2])
    assert np.array_equal(cutree(Tree(merge, height), k=3), [1, 2, 1, 3, 2])
    assert np.array_equal(cutree(Tree(merge, height), h=3.5), [1, 2, 1, 2, 2])
    # ward.D2 squares on the way in and reports the root
    m2, h2, _ = ref_hclust(d, "ward.D2")
    assert h2[0] == 1.0 and h2[1] == 2.0


def test_python_argument_checks():
    """Raised before the library (and so the GPU) is touched."""
    import scde_amd
    from scde_amd import cluster
    d = corr_dist(5)
    with pytest.raises(ValueError, match="square"):
        cluster.hclust(d[:, :4])
    with pytest.raises(ValueError, match="square"):
        cluster.hclust(np.zeros(4))
    for method in ("ward", "centroid", "median", "Ward.D"):
        with pytest.raises(ValueError) as e:
            cluster.hclust(d, method=method)
        assert all(m in str(e.value) for m in METHODS)
        with pytest.raises(ValueError, match="unknown method"):
            cluster.hclust_batch([d], method=method)
    with pytest.raises(ValueError, match="at least 2"):
        cluster.hclust(np.zeros((1, 1)))
    with pytest.raises(ValueError, match="at least 2"):
        cluster.hclust_batch([d, np.zeros((1, 1))])
    for f in ("hclust", "hclust_batch", "cutree", "pagoda_cluster_cells", "pagoda_gene_clusters_observed"):
        assert getattr(scde_amd, f) is getattr(cluster, f)


def test_earg_cases():
    """n < 2, ld < n, unknown method codes and null pointers are SCDE_EARG (1), checked before
    the device is looked for."""
    from scde_amd import _lib
    from scde_amd.api import _p
    L = _lib.lib()
    d = np.asfortranarray(corr_dist(4))
    merge, height, order = np.zeros((3, 2), np.int32, order="F"), np.zeros(3), np.zeros(4, np.int32)
    for f in (L.scde_hclust_host, L.scde_hclust_dev):
        assert f(None, _p(d), 4, 1, 0, _p(merge), _p(height), _p(order)) == 1
        assert b"at least 2" in L.scde_last_error()
        assert f(None, _p(d), 3, 4, 0, _p(merge), _p(height), _p(order)) == 1
        for code in (-1, 6, 7):
            assert f(None, _p(d), 4, 4, code, _p(merge), _p(height), _p(order)) == 1
            assert b"method" in L.scde_last_error()
        assert f(None, None, 4, 4, 0, _p(merge), _p(height), _p(order)) == 1
        assert f(None, _p(d), 4, 4, 0, _p(merge), None, _p(order)) == 1
        assert b"null" in L.scde_last_error()
    off, n = np.zeros(1, np.int64), np.array([1], np.int32)
    assert L.scde_hclust_batch_dev(None, 1, _p(d), _p(off), _p(n), 0, _p(merge), _p(height), _p(order)) == 1
    assert L.scde_hclust_batch_dev(None, 1, _p(d), None, _p(n), 0, _p(merge), _p(height), _p(order)) == 1


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error path")
def test_no_gpu_fails_loudly():
    from scde_amd import _lib, cluster
    with pytest.raises(_lib.ScdeError, match="device"):
        cluster.hclust(corr_dist(5))
    with pytest.raises(_lib.ScdeError, match="device"):
        cluster.hclust_batch([corr_dist(5), corr_dist(3)])


# ------------------------------------------------------------------ GPU tests
def _dev_put(a):
    from scde_amd import _lib, api
    L, ctx = _lib.lib(), api.default_context()
    p = ctypes.c_void_p()
    _lib.check(L.scde_dev_alloc(ctx.handle, a.nbytes, ctypes.byref(p)))
    _lib.check(L.scde_h2d(ctx.handle, p, api._p(a), a.nbytes))
    return p


def _dev_free(p):
    from scde_amd import _lib, api
    _lib.check(_lib.lib().scde_dev_free(api.default_context().handle, p))


def _c_entry(a, ld, n, method, dev):
    """scde_hclust_host / _dev on the buffer a (ld x n, column-major); (rc, HClust, bytes after)."""
    from scde_amd import _lib, api
    from scde_amd.cluster import HClust
    L, ctx = _lib.lib(), api.default_context()
    merge, height, order = np.zeros((n - 1, 2), np.int32, order="F"), np.zeros(n - 1), np.zeros(n, np.int32)
    after = None
    if dev:
        p = _dev_put(a)
        try:
            rc = L.scde_hclust_dev(ctx.handle, p, ld, n, METHODS.index(method), api._p(merge), api._p(height),
                                   api._p(order))
            msg = L.scde_last_error()
            after = np.empty_like(a)
            _lib.check(L.scde_d2h(ctx.handle, api._p(after), p, a.nbytes))
        finally:
            _dev_free(p)
    else:
        rc = L.scde_hclust_host(ctx.handle, api._p(a), ld, n, METHODS.index(method), api._p(merge), api._p(height),
                                api._p(order))
        msg = L.scde_last_error()
    return rc, msg, HClust(merge, height, order, method), after


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("method", METHODS)
def test_hclust_equals_restatement(method, n):
    from scde_amd import hclust
    got = hclust(corr_dist(n), method=method)
    assert got.method == method and got.labels is None
    assert got.merge.shape == (n - 1, 2) and sorted(got.order.tolist()) == list(range(1, n + 1))
    assert_same_tree(got, _ref("corr", n, method), f"{method} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["ward.D", "complete"])
def test_hclust_1500(method):
    """No multiple of anything, several strided passes per row."""
    from scde_amd import hclust
    assert_same_tree(hclust(corr_dist(1500, 8), method=method), _ref("corr8", 1500, method), f"{method} n=1500")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [40, 130])
@pytest.mark.parametrize("method", ["single", "complete", "average"])
def test_hclust_ties(method, n):
    """Integer distances in {1..4}: equal distances everywhere, decided by index -- what a
    nearest-neighbour cache that compares distances alone gets wrong."""
    from scde_amd import hclust
    assert_same_tree(hclust(tie_dist(n), method=method), _ref("tie", n, method), f"ties {method} n={n}")


@pytest.mark.gpu
def test_worked_example_and_labels():
    import pandas as pd

    from scde_amd import cutree, hclust
    d, merge, height, order = _five()
    names = ["a", "b", "c", "d", "e"]
    got = hclust(pd.DataFrame(d, index=names, columns=names), method="complete")
    assert got.labels == names
    assert np.array_equal(got.merge, merge) and np.array_equal(got.height, height)
    assert np.array_equal(got.order, order)
    assert np.array_equal(cutree(got, k=3), [1, 2, 1, 3, 2])


@pytest.mark.gpu
def test_triangle_and_stride():
    """Only the strict lower triangle is read: NaN over the diagonal and the upper triangle, and
    a leading dimension of n + 3 (NaN padding), change nothing; the device entry leaves the
    caller's buffer byte for byte as it was."""
    n = 65
    d = corr_dist(n)
    for method in ("ward.D", "single"):
        ref = _ref("corr", n, method)
        a = np.full((n + 3, n), np.nan, order="F")
        a[:n] = np.where(np.tri(n, k=-1, dtype=bool), d, np.nan)
        for dev in (False, True):
            rc, msg, got, after = _c_entry(a, n + 3, n, method, dev)
            assert rc == 0, msg
            assert_same_tree(got, ref, f"{method} lower triangle only, ld = n + 3, dev={dev}")
            if dev:
                assert after.tobytes() == a.tobytes()


@pytest.mark.gpu
def test_non_finite_values_are_refused():
    from scde_amd import _lib, hclust
    n = 70
    d = corr_dist(65)
    base = np.asfortranarray(corr_dist(n, seed=3))
    for (i, j), v in (((1, 0), np.nan), ((n - 1, n - 2), np.inf), ((40, 17), -np.inf)):
        a = base.copy(order="F")
        a[i, j] = v
        a[j, i] = 0.5  # the upper triangle is not looked at
        for dev in (False, True):
            rc, msg, _, after = _c_entry(a, n, n, "average", dev)
            assert rc == 1, (i, j, dev)
            assert f"row {i + 1}, column {j + 1}".encode() in msg, msg
            if dev:
                assert after.tobytes() == a.tobytes()
            # the context works on
            assert_same_tree(hclust(d, method="average"), _ref("corr", 65, "average"), "after a refusal")
        with pytest.raises(_lib.ScdeError, match="non-finite"):
            hclust(a, method="average")
    # several bad values: the first in column-major (as.dist) order is named
    a = base.copy(order="F")
    a[50, 3] = a[20, 5] = a[69, 2] = np.nan
    rc, msg, _, _ = _c_entry(a, n, n, "single", True)
    assert rc == 1 and b"row 70, column 3" in msg, msg


@pytest.mark.gpu
def test_batch():
    from scde_amd import _lib, hclust, hclust_batch
    sizes = [2, 65, 300, 1025, 64]
    ds = [corr_dist(n) for n in sizes]
    for method in ("ward.D", "mcquitty"):
        got = hclust_batch(ds, method=method)
        assert len(got) == len(sizes)
        for n, g, d in zip(sizes, got, ds):
            one = hclust(d, method=method)
            assert np.array_equal(g.merge, one.merge) and np.array_equal(g.height, one.height)
            assert np.array_equal(g.order, one.order), (method, n)
    # more workgroups than compute units
    many = [corr_dist(33, seed=100 + p) for p in range(300)]
    got = hclust_batch(many, method="ward.D")
    for p, (g, d) in enumerate(zip(got, many)):
        assert_same_tree(g, ref_hclust(d, "ward.D"), f"batch of 300, problem {p}")  # (usable: CPU test below)
    assert hclust_batch([]) == []
    bad = [d.copy() for d in ds[:3]]
    bad[2][7, 4] = np.nan
    with pytest.raises(_lib.ScdeError, match=r"problem 2: non-finite distance at row 8, column 5"):
        hclust_batch(bad, method="ward.D")
    assert_same_tree(hclust_batch(ds[:2], method="ward.D")[1], _ref("corr", 65, "ward.D"), "batch after a refusal")


MODEL_COLUMNS = ["conc.b", "conc.a", "fail.r", "corr.b", "corr.a", "corr.theta", "corr.ltheta.b", "corr.ltheta.t",
                 "corr.ltheta.m", "corr.ltheta.s", "corr.ltheta.r", "conc.a2"]


@pytest.mark.gpu
def test_hclust_of_reciprocal_distance():
    """The chain the distances were built for: reciprocal_distance -> hclust, on the fixture."""
    from scde_amd import cutree, hclust, reciprocal_distance
    g = golden("esmef500.npz")
    mm = g["models"]
    models = {c: mm[:, j] for j, c in enumerate(MODEL_COLUMNS) if not np.all(np.isnan(mm[:, j]))}
    d = reciprocal_distance(models, np.ascontiguousarray(g["counts"]))
    assert np.isfinite(d).all()
    got = hclust(d, method="ward.D")
    assert_same_tree(got, ref_checked(d, "ward.D"), "ward.D of the reciprocal distance")
    lab = cutree(got, k=3)
    assert lab[0] == 1 and set(lab.tolist()) == {1, 2, 3}


def _cells_varinfo():
    rng = np.random.default_rng(21)
    ng, nc = 60, 40
    genes = [f"g{i}" for i in range(ng)]
    mat = rng.normal(size=(ng, nc))
    matw = rng.uniform(0.05, 1.0, size=(ng, nc))
    arv = rng.uniform(0.5, 1.5, ng) / matw.sum(1)  # rowSums(matw) * arv straddles 1
    gw = {genes[i]: float(rng.uniform(0.5, 2)) for i in rng.choice(ng, 30, replace=False)}
    tam = {"gw": gw, "xv": rng.normal(size=(3, nc)), "xvw": rng.uniform(0.2, 1.0, size=(3, nc))}
    return tam, {"mat": mat, "matw": matw, "arv": arv, "genes": genes, "cells": [f"c{i}" for i in range(nc)]}


@pytest.mark.gpu
def test_pagoda_cluster_cells():
    from scde_amd import pagoda, pagoda_cluster_cells
    tam, vi = _cells_varinfo()
    od = vi["matw"].sum(1) * vi["arv"]
    keep = [g for g in tam["gw"] if od[vi["genes"].index(g)] > 1]
    assert 5 < len(keep) < 30
    rows = [vi["genes"].index(g) for g in keep]
    for aspects in (False, True):
        m, w = vi["mat"][rows], vi["matw"][rows]
        if aspects:
            m, w = np.vstack([m, tam["xv"]]), np.vstack([w, tam["xvw"]])
        dm = 1 - pagoda.matWCorr(m, w)
        assert np.isfinite(np.tril(dm, -1)).all()
        for method in ("ward.D", "complete"):
            res = pagoda_cluster_cells(tam, vi, method=method, include_aspects=aspects, return_details=True)
            assert res["genes"] == keep
            assert np.array_equal(res["distance"], dm)
            assert_same_tree(res["clustering"], ref_checked(dm, method), f"cluster.cells {method} aspects={aspects}")
            assert res["clustering"].labels == vi["cells"]
            hc = pagoda_cluster_cells(tam, vi, method=method, include_aspects=aspects)
            assert np.array_equal(hc.merge, res["clustering"].merge)
    stricter = pagoda_cluster_cells(tam, vi, min_overdispersion=1.2, return_details=True)
    assert stricter["genes"] == [g for g in tam["gw"] if od[vi["genes"].index(g)] > 1.2]


def _close_cols(a, b, rel, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    scale = np.maximum(np.abs(a).max(0), np.abs(b).max(0))
    err = np.abs(a - b).max(0)
    assert np.all(err <= rel * scale + 1e-300), f"{what}: max err {err} vs scale {scale}"


def _genes_varinfo():
    rng = np.random.default_rng(33)
    ng, nc = 200, 50
    load = rng.normal(size=(ng, 4)) * (rng.random((ng, 4)) < 0.4)
    mat = load @ rng.normal(size=(4, nc)) + 0.7 * rng.normal(size=(ng, nc))
    mat[[17, 120]] = 1.25  # constant rows
    matw = rng.uniform(0.1, 1.0, size=(ng, nc))
    return {"mat": mat, "matw": matw, "genes": [f"g{i}" for i in range(ng)]}


@pytest.mark.gpu
@pytest.mark.parametrize("trim", [0, None])
def test_pagoda_gene_clusters_observed(trim):
    from scde_amd import cutree, pagoda, pagoda_gene_clusters_observed
    vi = _genes_varinfo()
    res = pagoda_gene_clusters_observed(vi, trim=trim, n_clusters=8, n_starts=3, seed=5, return_details=True)
    nc = vi["mat"].shape[1]
    assert res["trim"] == (0 if trim == 0 else 3.1 / nc)
    mat = vi["mat"] if trim == 0 else np.asarray(pagoda.winsorize_matrix(vi["mat"], 3.1 / nc))
    kept = [g for i, g in enumerate(vi["genes"]) if i not in (17, 120)]
    assert res["genes"] == kept  # the constant rows are dropped
    rows = [vi["genes"].index(g) for g in kept]
    # the bar tests/test_gpu_pagoda.py applies to matCorr
    np.testing.assert_allclose(res["distance"], 1 - np.corrcoef(mat[rows]), rtol=1e-11, atol=1e-14)
    assert np.isfinite(res["distance"]).all()
    tree = ref_checked(res["distance"], "ward.D")
    assert_same_tree(res["clustering"], tree, "gene clusters")
    lab = cutree(Tree(tree[0], tree[1]), k=8)
    assert list(res["clusters"]) == [f"geneCluster.{c}" for c in range(1, 9)] == list(res["cl.goc"])
    rs = pagoda.RState(5)
    for c in range(1, 9):
        genes = [g for g, l in zip(kept, lab) if l == c]
        assert res["clusters"][f"geneCluster.{c}"] == genes
        ii = [vi["genes"].index(g) for g in genes]
        one = pagoda.bwpca(mat[ii].T, vi["matw"][ii].T, npcs=1, nstarts=3, center=False, rstate=rs)
        cs = np.sign(pagoda._r_cor(one["scores"][:, 0], (mat[ii] * np.abs(one["rotation"][:, 0])[:, None]).mean(0)))
        got = res["cl.goc"][f"geneCluster.{c}"]
        assert got["n"] == len(ii)
        what = f"geneCluster.{c}"
        # tests/test_gpu_wpca.py's batch-against-single bar
        _close_cols(got["xp"]["rotation"], one["rotation"] * cs, 1e-7, what + " rotation")
        _close_cols(got["xp"]["scores"], one["scores"] * cs, 1e-7, what + " scores")
        _close_cols(got["xp"]["scoreweights"], one["scoreweights"], 1e-9, what + " scoreweights")
        np.testing.assert_allclose(got["xp"]["var"], one["var"], rtol=1e-8, err_msg=what)
        assert got["xp"]["totvar"] == pytest.approx(one["totvar"], rel=1e-12)
        np.testing.assert_allclose(got["sd"], np.sqrt(one["var"])[None, :], rtol=1e-8)
    plain = pagoda_gene_clusters_observed(vi, trim=trim, n_clusters=8, n_starts=3, seed=5)
    assert set(plain) == {"clusters", "cl.goc", "trim"} and plain["clusters"] == res["clusters"]
