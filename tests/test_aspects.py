"""CPU tests of PAGODA's aspect redundancy reduction: the restatement in tests/aspects_ref.py
against mpmath, and the host side of scde_amd/aspects.py (name parsing, loading lists, the
``cnam`` bookkeeping, the variance order, argument checks, and that nothing is computed without
a GPU).  The GPU tests are in tests/test_gpu_aspects.py."""
import numpy as np
import pytest

import aspects_ref as R
from conftest import gpu_available


@pytest.fixture(scope="module")
def A():
    from scde_amd import aspects
    return aspects


# ------------------------------------------------------------------ the renormalisation
def test_restatement_against_mpmath_on_the_grid():
    """The float64 restatement's own error on the grid n x r of the issue, where its log p is
    finite: the figure the GPU test's bar scales.  Its formula is the correlation-space reading of
    the contract through scipy.special's incomplete beta function and its inverse, good to a few
    ulp of 1; a literal restatement through scipy.stats.t is off by up to 2e-7 deep in the tail
    (n = 101, r = 0.999999) and is kept only to pin the deviation."""
    worst, deep = 0.0, 0
    for n in R.GRID_N:
        for r in R.GRID_R:
            for s in (1.0, -1.0):
                ex, f64 = R.t_renorm_exact(r, n) * s, R.t_renorm64(s * r, n)
                if r == 0:
                    assert f64 == 0 and ex == 0
                elif np.isfinite(R.t_renorm_logp(r, n)):
                    worst = max(worst, abs(ex - f64))
                else:
                    deep += 1
                    assert abs(ex) > 0.99  # p has underflowed: |cr| is 1 to a few ulp
    print(f"restatement's own maximum error on the grid: {worst:.3g}; {deep} points beyond its log p")
    assert worst < 64 * R.U   # a few ulp of 1: scipy's incomplete beta function and its inverse
    assert deep >= 8


def test_exact_r_cases_and_same_ndf():
    for f in (R.t_renorm64, R.t_renorm_exact):
        for n in (0, 1, 2):
            assert f(0.3, n) == 0.3 and f(-0.7, n) == -0.7
        assert f(1.0, 50) == 1.0 and f(-1.0, 50) == -1.0
        assert np.isnan(f(float("nan"), 50))
        assert f(0.0, 50) == 0.0
    # nu = n - 2 on one side, target_ndf - 2 on the other: n = target_ndf is the identity
    for r in (1e-8, 0.1, -0.5, 0.9, 0.999999):
        assert abs(R.t_renorm_exact(r, 100, 100) - r) <= R.U * abs(r)
        assert abs(R.t_renorm_exact(r, 102, 102) - r) <= R.U * abs(r)
        assert abs(R.t_renorm64(r, 100, 100) - r) <= 64 * R.U
    # (n = 102 against target_ndf = 100 compares 100 with 98 degrees of freedom: not the identity)
    assert abs(R.t_renorm_exact(0.5, 102, 100) - 0.5043923469008006) < 1e-15


def test_literal_R_lines_lose_the_negative_side():
    """R/functions.R:5148-5152 in float64: for a strongly negative r the upper tail is 1 to
    rounding, qt gives -Inf, nr is NaN and r is kept; the contract is the odd map."""
    assert R.t_renorm_R(-0.9, 2000) == -0.9
    assert R.t_renorm64(-0.9, 2000) < -0.999
    assert R.t_renorm_exact(-0.9, 2000) == -R.t_renorm_exact(0.9, 2000)


def test_matrix_form_mirrors_and_keeps_the_diagonal():
    r = np.array([[1.0, 0.5, 9.0], [9.0, 1.0, -0.2], [9.0, 9.0, 1.0]])
    n = np.array([[0, 30, 0], [0, 0, 40], [0, 0, 0]])
    r[0, 2], n[0, 2] = 0.1, 2
    cr = R.t_renorm_matrix(r, n, 100)
    assert np.array_equal(cr, cr.T) and np.array_equal(np.diag(cr), np.ones(3))
    assert cr[0, 2] == 0.1 and cr[0, 1] == R.t_renorm64(0.5, 30) and cr[1, 2] == R.t_renorm64(-0.2, 40)


# ------------------------------------------------------------------ names and loading lists
def pcc_small():
    rot = lambda *cols: np.column_stack(cols)  # noqa: E731
    return {
        "setA": {"xp": {"rotation": rot([1.0, 2.0, 4.0], [0.5, -1.0, 0.25]), "rotation_names": ["g3", "g1", "g2"]}},
        "odd # name": {"xp": {"rotation": rot([1.0, -1.0, 3.0, 0.0]), "rotation_names": ["g2", "g9", "g3", "g7"]}},
        "geneCluster.1": {"xp": {"rotation": rot([2.0, 1.0]), "rotation_names": ["g7", "g5"]}},
    }


NAMES = ["#PC1# setA", "#PC1# odd # name", "#PC2# setA", "#PC1# geneCluster.1"]


def test_name_parsing(A):
    assert A.parse_aspect_names(NAMES) == [("setA", 1), ("odd # name", 1), ("setA", 2), ("geneCluster.1", 1)]
    assert A.parse_aspect_names(["#PC12# #PC1# x"]) == [("#PC1# x", 12)]
    assert A.parse_aspect_names(NAMES) == R.parse_names(NAMES)
    with pytest.raises(ValueError, match="not of the form"):
        A.parse_aspect_names(["PC1 setA"])


def test_rotn_order_and_lists(A):
    pcc = pcc_small()
    rotn, pl = A.loading_lists(pcc, NAMES)
    assert rotn == ["g3", "g1", "g2", "g9", "g7", "g5"]  # first appearance, aspects in order
    rr, pr = R.loading_lists(pcc, NAMES)
    assert rr == rotn
    for (i, v), (ri, rv) in zip(pl, pr):
        assert np.array_equal(i, ri) and np.array_equal(v, rv)
    i, v = pl[1]  # g2, g9, g3, g7 -> indices 2, 3, 0, 4, ordered 0, 2, 3, 4; centred by the column's own mean
    assert list(i) == [0, 2, 3, 4] and np.array_equal(v, np.array([3.0, 1.0, -1.0, 0.0]) - 0.75)
    assert list(pl[2][0]) == [0, 1, 2] and np.allclose(pl[2][1], np.array([0.5, -1.0, 0.25]) + 1 / 12)
    with pytest.raises(ValueError, match="component"):
        A.loading_lists(pcc, ["#PC3# setA", "#PC1# setA"])
    with pytest.raises(ValueError, match="no principal components"):
        A.loading_lists(pcc, ["#PC1# nope", "#PC1# setA"])
    # c(pwpca, clpca$cl.goc): the first of a name wins
    merged = A._merge_pcc({"setA": pcc["setA"]}, {"cl.goc": {"setA": pcc["odd # name"], "k": pcc["geneCluster.1"]}})
    assert merged["setA"] is pcc["setA"] and merged["k"] is pcc["geneCluster.1"]


def test_pl_cor_restatement():
    pl = R.loading_lists(pcc_small(), NAMES)[1]
    r, n = R.pl_cor(pl)
    assert n[0, 1] == 3 + 4 - 2 and n[0, 3] == 5 and r[0, 3] == 0   # nothing shared: 0
    assert n[1, 3] == 4 + 2 - 1 and abs(r[1, 3]) == 1                # one shared gene: +-1
    assert np.array_equal(r, r.T) and np.array_equal(np.diag(r), np.ones(4))


# ------------------------------------------------------------------ cnam, order, top
def test_cnam_merging(A):
    names = ["a", "b", "c", "d"]
    members = [np.array([0, 2]), np.array([1]), np.array([3])]
    rn = ["c", "b", "d"]
    assert A._cnam({}, names, members, rn) == {"c": ["a", "c"], "b": ["b"], "d": ["d"]}
    old = {"cnam": {"a": ["a1", "a2"], "c": ["c1"], "b": ["b1"]}}  # (d has none: unlist() drops it)
    got = A._cnam(old, names, members, rn)
    assert got == {"c": ["a1", "a2", "c1"], "b": ["b1"], "d": []} and list(got) == rn
    assert got == R.cnam(old["cnam"], names, members, rn)


def test_variance_order_is_stable_and_top():
    d = np.array([[0.0, 1.0, 2.0], [0.0, 2.0, 4.0], [2.0, 1.0, 0.0], [5.0, 5.0, 5.0], [4.0, 2.0, 0.0]])
    assert list(R.variance_order(d)) == [1, 4, 0, 2, 3]     # ties keep their order
    assert list(R.variance_order(d, 2)) == [1, 4]
    assert list(R.variance_order(d, 50)) == [1, 4, 0, 2, 3]


def test_winsorize_and_cut_restatements():
    x = np.array([[5.0, 1.0, 3.0, 2.0, 4.0]])
    assert np.array_equal(R.winsorize_rows(x, 0.2), [[4.0, 2.0, 3.0, 2.0, 4.0]])
    assert np.array_equal(R.winsorize_rows(x, 1), [[4.0, 2.0, 3.0, 2.0, 4.0]])  # above 0.5: a count
    d = np.array([[0, .1, .9, .8], [.1, 0, .85, .9], [.9, .85, 0, .05], [.8, .9, .05, 0]])
    assert list(R.cut_complete(d, 0.2)) == [1, 1, 2, 2]
    assert list(R.cut_complete(d[::-1, ::-1], 0.01)) == [1, 2, 3, 4]


def test_collapse_restatement_small():
    rows = np.array([[1.0, 2.0, 4.0, 3.0], [2.0, 4.0, 8.5, 6.0], [5.0, 5.0, 5.0, 5.0]])
    col = R.collapse(rows, np.ones_like(rows), [1, 1, 2], ["a", "b", "c"])
    assert col["names"] == ["b", "c"] and np.array_equal(col["d"][1], rows[2])
    assert abs(np.var(col["d"][0], ddof=1) - np.var(rows[1], ddof=1)) < 1e-12   # scaled to the top row
    assert col["orientation"][0] > 0.99 and np.allclose(col["w"][0], 0.25)
    ex = R.collapse(rows, np.ones_like(rows), [1, 1, 2], ["a", "b", "c"], exact=True)
    assert float(np.abs(ex["d"][0] - col["d"][0]).max()) < 1e-13
    fb = R.collapse(np.full((2, 4), 3.0), np.ones((2, 4)), [1, 1], ["a", "b"], seed=3)
    assert fb["fallback"] == [True] and np.allclose(fb["d"][0], np.abs(R.r_rnorm(3, 4)) * 1e-6)
    # R's stream: set.seed(1); rnorm(3) is -0.6264538 0.1836433 -0.8356286
    assert np.allclose(R.r_rnorm(1, 3), [-0.6264538, 0.1836433, -0.8356286], atol=5e-8, rtol=0)


# ------------------------------------------------------------------ argument checks, no GPU
def tam_small():
    rng = np.random.default_rng(0)
    return {"xv": rng.normal(size=(4, 6)), "xvw": np.ones((4, 6)), "names": list(NAMES)}


def test_argument_checks(A):
    tam, pcc = tam_small(), pcc_small()
    one = {"xv": tam["xv"][:1], "xvw": tam["xvw"][:1], "names": NAMES[:1]}
    with pytest.raises(ValueError, match="at least 2 aspects"):
        A.pagoda_reduce_loading_redundancy(one, pcc)
    with pytest.raises(ValueError, match="at least 2 aspects"):
        A.pagoda_reduce_redundancy(one)
    with pytest.raises(ValueError, match="at least 2 aspects"):
        A.pathway_pc_correlation_distance(pcc, NAMES[:1])
    with pytest.raises(ValueError, match="unknown method"):
        A.pagoda_reduce_redundancy(tam, cluster_method="centroid")
    with pytest.raises(ValueError, match="unknown method"):
        A.pagoda_reduce_loading_redundancy(tam, pcc, cluster_method="median")
    with pytest.raises(ValueError, match="same shape"):
        A.pagoda_reduce_redundancy({**tam, "xvw": np.ones((4, 5))})
    with pytest.raises(ValueError, match="names"):
        A.pagoda_reduce_redundancy({**tam, "names": NAMES[:3]})
    with pytest.raises(ValueError, match="4 x 4"):
        A.pagoda_reduce_redundancy(tam, distance=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="top"):
        A.pagoda_reduce_redundancy(tam, top=0)
    with pytest.raises(ValueError, match="trim"):
        A.pagoda_reduce_redundancy(tam, trim=-1)
    with pytest.raises(ValueError, match="target_ndf"):
        A.pathway_pc_correlation_distance(pcc, NAMES, target_ndf=2)
    with pytest.raises(ValueError, match="one entry per aspect"):
        A.collapse_aspect_clusters(tam["xv"], tam["xvw"], [1, 1, 2], NAMES)
    with pytest.raises(ValueError, match="same shape"):
        A.collapse_aspect_clusters(tam["xv"], tam["xvw"][:, :3], [1, 1, 2, 2], NAMES)


def test_exports():
    import scde_amd
    for f in ("pathway_pc_correlation_distance", "collapse_aspect_clusters", "pagoda_reduce_loading_redundancy",
              "pagoda_reduce_redundancy"):
        assert callable(getattr(scde_amd, f))


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error path")
def test_every_function_fails_loudly_without_a_gpu(A):
    from scde_amd._lib import ScdeError
    tam, pcc = tam_small(), pcc_small()
    with pytest.raises(ScdeError):
        A.pathway_pc_correlation_distance(pcc, NAMES, target_ndf=100)
    with pytest.raises(ScdeError):
        A.collapse_aspect_clusters(tam["xv"], tam["xvw"], [1, 1, 2, 2], NAMES)
    with pytest.raises(ScdeError):
        A.pagoda_reduce_loading_redundancy(tam, pcc)
    with pytest.raises(ScdeError):
        A.pagoda_reduce_redundancy(tam)
