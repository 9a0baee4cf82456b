"""The numpy restatement of the views (tests/views_ref.py) on its own: the branches, the flip
rule, the name matching, and the walkthrough's point -- the pattern ``pagoda.show.pathways``
returns, handed to ``pagoda.subtract.aspect``, takes the planted aspect out.  No GPU.

The synthetic case (240 genes x 96 cells, two overlapping gene sets carrying one planted cell
pattern, a third set carrying none, two batch levels) is planted strongly enough that the loading
of the last gene kept and of the first one left out differ by far more than a rounding; that gap
is asserted here, so the discrete results tests/test_gpu_views.py compares (which genes, which
trees) cannot hinge on one."""
import math
import warnings

import numpy as np
import pytest

import views_ref as V
from oracle import wpca as W
from varnorm_ref import subtract_aspect

GAP = 1e-6  # relative


@pytest.fixture(scope="module")
def case():
    return V.make_case()


@pytest.fixture(scope="module")
def both(case):
    varinfo, goenv, _ = case
    return V.show_pathways(["GO:A", "GO:B"], varinfo, goenv)


def rel_gap(a, b):
    return abs(a - b) / max(abs(a), abs(b))


def test_selection_gaps(case):
    varinfo, goenv, _ = case
    names = list(varinfo["genes"])
    # several pathways, one- and two-sided, at the n_genes the GPU tests use
    pathways, p_genes = V.match_names(["GO:A", "GO:B"], names, goenv)
    for trim in (0, 2.1 / V.C):
        ppca, _ = V.pathway_pcas(varinfo, p_genes, 1, trim)
        sn, sv = V.scaled_loadings(ppca, pathways, [1, 1])
        red = V.reduced(sn, np.abs(sv), max, True)
        assert len(red) == 50
        print(f"several, trim {trim:.3g}: |loading| 20th, 21st:", red[19][1], red[20][1])
        assert rel_gap(red[19][1], red[20][1]) > GAP
        for how, dec in ((max, True), (min, False)):
            r = V.reduced(sn, sv, how, dec)
            assert rel_gap(r[9][1], r[10][1]) > GAP
        # no two adjacent values of the whole ranking are a rounding apart either (any n_genes)
        v = np.array([x for _, x in red])
        assert np.all(np.abs(np.diff(v)) > GAP * v[:-1])
    # one pathway
    for p in ("GO:A", "GO:B", "GO:C"):
        _, pg = V.match_names([p], names, goenv)
        r = V.pathway_pcas(varinfo, pg, 2)[0][p]
        for k in (0, 1):
            a = np.sort(np.abs(r["xp"]["rotation"][:, k]))[::-1]
            assert np.all(np.abs(np.diff(a)) > GAP * a[:-1]), (p, k)


def test_several_pathways_branch(case, both):
    varinfo, goenv, pattern = case
    assert both["consensus_pc"] == 1 and len(both["lab"]) == 20
    assert set(both["lab"]) <= set(V.SET_A) | set(V.SET_B)
    assert both["rotation"].shape == (20, 1) and both["scores"].shape == (V.C, 1)
    assert both["vmap"].shape == (20, V.C) and sorted(both["row_order"]) == list(range(1, 21))
    assert both["zlim"][0] < 0 < both["zlim"][1]
    assert both["vmap"].min() == both["zlim"][0] and both["vmap"].max() == both["zlim"][1]
    assert both["hc"][0].shape == (19, 2) and both["vhc"][0].shape == (V.C - 1, 2)
    # the consensus pattern is the planted one
    assert abs(V.r_cor(both["oc"], pattern)) > 0.95
    np.testing.assert_array_equal(both["oc"], both["scores"][:, 0])


def test_one_pathway_branch(case):
    varinfo, goenv, pattern = case
    one = V.show_pathways(["GO:A"], varinfo, goenv, n_genes=12)
    assert one["consensus_pc"] == 1 and len(one["lab"]) == 12 and one["rotation"].shape[0] == 12
    a = np.abs(one["rotation"][:, 0])
    assert np.all(np.diff(a) < 0)  # the genes kept, by decreasing |loading|
    assert abs(V.r_cor(one["oc"], pattern)) > 0.95
    # n_genes above the pathway's size keeps all of it, the rotation left in matrix order
    full = V.show_pathways(["GO:A"], varinfo, goenv, n_genes=100)
    assert len(full["lab"]) == 30 and full["rotation_names"] == V.SET_A
    # the second component of a pathway
    pc2 = V.show_pathways(["GO:A"], varinfo, goenv, n_genes=12, n_pc=[2])
    assert pc2["consensus_pc"] == 2 and pc2["scores"].shape[1] == 2
    np.testing.assert_array_equal(pc2["oc"], pc2["scores"][:, 1])


def test_two_sided(case):
    varinfo, goenv, _ = case
    two = V.show_pathways(["GO:A", "GO:B"], varinfo, goenv, n_genes=20, two_sided=True)
    # every fourth planted gene loads against the rest: one sign supplies at most 10 genes
    neg = {f"g{i}" for i in range(50) if i % 4 == 3}
    n_neg = len(set(two["lab"]) & neg)
    assert len(two["lab"]) == 20 and n_neg in (10, 20 - 10) and len(set(two["lab"])) == 20
    one = V.show_pathways(["GO:A", "GO:B"], varinfo, goenv, n_genes=20)
    assert set(one["lab"]) != set(two["lab"])
    # the first occurrence of a name is kept
    assert V.select(["a", "b", "c"], np.array([3.0, -2.0, 1.0]), 4, True) == ["a", "c", "b"]
    assert V.select(["a", "b", "a"], np.array([1.0, -2.0, -3.0]), 2, True) == ["a"]
    # ties go by the sorted names
    assert V.select(["z", "y", "x"], np.array([1.0, 1.0, 1.0]), 2, False) == ["x", "y"]


def test_fewer_than_three_genes(case):
    varinfo, goenv, _ = case
    assert V.show_pathways(["GO:A", "GO:B"], varinfo, goenv, n_genes=2) is None
    assert V.show_pathways(["GO:A", "GO:B"], varinfo, goenv, n_genes=3) is not None
    two = V.show_pathways(["g1", "g2"], varinfo, goenv)  # one "pathway" of two genes: no tree
    assert two["hc"] is None and list(two["row_order"]) == [1, 2]


def test_gene_names_against_pathway_names(case):
    varinfo, goenv, _ = case
    genes = V.SET_A[:15]
    by_gene = V.show_pathways(genes, varinfo, goenv)
    by_set = V.show_pathways(["S"], varinfo, {"S": genes})
    assert by_gene["lab"] == by_set["lab"]
    np.testing.assert_array_equal(by_gene["oc"], by_set["oc"])
    # a pathway name wins over a gene of the same name
    assert V.match_names(["g1"], varinfo["genes"], {"g1": ["g2", "g3"]}) == (["g1"], {"g1": ["g2", "g3"]})
    with pytest.raises(ValueError, match="do not match either gene nor pathway names"):
        V.show_pathways(["nothing"], varinfo, goenv)
    with pytest.raises(ValueError):
        V.show_pathways(["GO:A"], varinfo, None)


def test_partial_match_warns(case):
    varinfo, goenv, _ = case
    with pytest.warns(UserWarning, match="partial match to pathway names.*GO:nope"):
        got = V.show_pathways(["GO:A", "GO:nope"], varinfo, goenv, n_genes=12)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ref = V.show_pathways(["GO:A"], varinfo, goenv, n_genes=12)
    np.testing.assert_array_equal(got["oc"], ref["oc"])
    with pytest.warns(UserWarning, match="partial match to gene names.*nope"):
        V.show_pathways(["g1", "g2", "g3", "nope"], varinfo, goenv)


def test_flip_rule(case, both):
    assert V.flips(-1e-300) and not V.flips(0.0) and not V.flips(1e-300) and not V.flips(math.nan)
    # after the flip the pattern never runs against the mean expression
    assert V.r_cor(both["oc"], both["aval"]) >= 0
    varinfo, goenv, _ = case
    t = V.pathway_genes(["GO:A"], varinfo, goenv)
    assert V.spearman(t["oc"], t["aval"]) >= 0
    # the sign of the input decides nothing: mirrored data gives the mirrored loadings, the same pattern sign
    mirrored = dict(varinfo, mat=-np.asarray(varinfo["mat"]))
    m = V.show_pathways(["GO:A", "GO:B"], mirrored, goenv)
    assert V.r_cor(m["oc"], m["aval"]) >= 0
    # Spearman and Pearson can disagree: one far outlier
    x = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    y = np.array([6.0, 5.0, 4.0, 3.0, 2.0, 100.0])
    assert V.r_cor(x, y) > 0 > V.spearman(x, y)
    # and an exactly zero Spearman correlation, which does not flip
    assert V.spearman(x[:5], [5.0, 4.0, 3.0, 2.0, 100.0]) == 0.0
    assert V.spearman([1.0, 2.0, 3.0], [1.0, 2.0, 1.0]) == 0.0


def test_pathway_genes(case):
    varinfo, goenv, pattern = case
    t = V.pathway_genes(["GO:A"], varinfo, goenv)
    assert t["lab"] == list(range(30)) and t["rotation"].shape == (30, 1)
    assert abs(V.r_cor(t["oc"], pattern)) > 0.95
    assert V.pathway_genes(["g3", "g1"], varinfo, goenv)["lab"] == [1, 3]  # matrix order; no PCA below 3
    assert "scores" not in V.pathway_genes(["g3", "g1"], varinfo, goenv)
    assert V.pathway_genes(["nothing"], varinfo, goenv) is None


def test_view_aspects():
    rng = np.random.default_rng(3)
    xv = rng.normal(size=(7, 40)) * np.array([1, 5, 2, 5, 3, 0.5, 4])[:, None]
    xv[3] = xv[1][::-1]  # the same variance as row 1 up to rounding of the sum's order
    full = V.view_aspects(xv)
    assert list(full["vi"]) == list(range(7)) and full["row_clustering"][0].shape == (6, 2)
    assert full["mat"].max() == full["zlim"][1] == -full["zlim"][0]
    top3 = V.view_aspects(xv, top=3)
    assert set(top3["vi"]) == {1, 3, 6} and np.all(np.diff(top3["rcmvar"]) <= 0)
    assert V.view_aspects(xv, top=1)["row_clustering"] is None
    assert list(V.view_aspects(xv, top=100)["vi"]) == list(np.argsort(-np.var(xv, axis=1, ddof=1), kind="stable"))


def test_subtracting_the_pattern_removes_the_aspect(case, both):
    """vignettes/pagoda.md: cc.pattern <- pagoda.show.pathways(...); pagoda.subtract.aspect(varinfo, cc.pattern)."""
    varinfo, goenv, _ = case
    kw = dict(n_components=1, min_pathway_size=0, n_randomizations=0, n_starts=2, batch=varinfo["batch"])
    before = W.pagoda_pathway_wPCA(varinfo["mat"], varinfo["matw"], varinfo["genes"], goenv, **kw)
    mat2 = subtract_aspect(np.asarray(varinfo["mat"]), np.asarray(varinfo["matw"]), both["scores"][:, 0])
    after = W.pagoda_pathway_wPCA(mat2, varinfo["matw"], varinfo["genes"], goenv, **kw)
    for p in ("GO:A", "GO:B"):
        print(p, "PC1 sd before", before[p]["sd"][0, 0], "after", after[p]["sd"][0, 0])
        assert after[p]["sd"][0, 0] < before[p]["sd"][0, 0]
    assert after["GO:A"]["sd"][0, 0] < 0.5 * before["GO:A"]["sd"][0, 0]
