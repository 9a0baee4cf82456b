"""The Spearman restatement (tests/spearman_ref.py) against scipy, its NaN cases built by hand,
and the argument errors of the new keywords.  No GPU."""
import math

import numpy as np
import pytest

import spearman_ref as S
from conftest import golden

NAN = float("nan")


@pytest.mark.parametrize("thr", [1, 2, 5])
def test_pair_similarity_against_scipy(thr):
    """rankdata + pearsonr on the complete cases.  1e-13 absolute: scipy's two-pass sums carry
    about m 2^-53 with m <= 300; 2.2e-16 was seen."""
    from scipy.stats import pearsonr, rankdata
    counts = golden("knn300.npz")["counts"]
    worst, ms = 0.0, []
    for i in range(24):
        for j in range(i + 1, 24):
            s = S.common_genes(counts[:, i], counts[:, j], thr)
            ms.append(len(s))
            got = S.pair_similarity(counts[:, i], counts[:, j], thr)
            x, y = np.sqrt(counts[s, i].astype(np.float64)), np.sqrt(counts[s, j].astype(np.float64))
            ref = pearsonr(rankdata(x, method="average"), rankdata(y, method="average"))[0]
            assert not math.isnan(got) and not math.isnan(ref), (i, j)
            worst = max(worst, abs(got - ref))
    print(f"thr {thr}: m from {min(ms)} to {max(ms)}, max |restated - scipy| = {worst:.3g}")
    assert worst <= 1e-13


def test_rank_against_scipy():
    from scipy.stats import rankdata
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 17, 200):
        for v in (rng.normal(size=n), rng.integers(0, 4, n).astype(np.float64), np.full(n, 2.5)):
            assert np.array_equal(S.rank(v), rankdata(v, method="average"))
    v = np.array([0.0, -0.0, 1.0, -1.0, -0.0, np.inf, -np.inf, np.inf])
    assert np.array_equal(S.rank(v), rankdata(v, method="average"))
    assert S.rank(v)[0] == S.rank(v)[1] == S.rank(v)[4] == 4.0  # -0.0 ties with 0.0
    w = np.array([3.0, NAN, 1.0, 3.0, NAN, -np.inf])
    got = S.rank(w)
    ok = ~np.isnan(w)
    assert np.array_equal(np.isnan(got), ~ok)  # NaN kept
    assert np.array_equal(got[ok], rankdata(w[ok], method="average"))
    assert np.array_equal(got[ok], [3.5, 2.0, 3.5, 1.0])
    x = rng.normal(size=(9, 4))
    x[2, 1] = NAN
    r = S.rank_columns(x)
    for j in range(4):
        assert np.array_equal(r[:, j], S.rank(x[:, j]), equal_nan=True)


def nan_cases():
    """name -> (cell i, cell j, thr): pairs whose similarity is NaN by the contract."""
    return {
        # no gene valid in both
        "m0": (np.array([4, 0, 7, 0, 2], np.int32), np.array([0, 3, 0, 9, 0], np.int32), 1),
        # exactly one
        "m1": (np.array([4, 0, 7, 0, 2], np.int32), np.array([0, 3, 5, 9, 0], np.int32), 1),
        # four common genes, all tied in cell i although cell i's whole column is not constant
        "tied": (np.array([6, 6, 2, 6, 6, 9], np.int32), np.array([1, 5, 0, 3, 8, 0], np.int32), 1),
    }


def test_nan_cases_are_what_they_claim():
    cases = nan_cases()
    ci, cj, thr = cases["m0"]
    assert len(S.common_genes(ci, cj, thr)) == 0 and (ci >= thr).any() and (cj >= thr).any()
    ci, cj, thr = cases["m1"]
    assert len(S.common_genes(ci, cj, thr)) == 1
    ci, cj, thr = cases["tied"]
    s = S.common_genes(ci, cj, thr)
    assert len(s) == 4 and len(set(ci[s])) == 1 and len(set(cj[s])) == 4 and len(set(ci[ci >= thr])) > 1
    for name, (ci, cj, thr) in cases.items():
        assert math.isnan(S.pair_similarity(ci, cj, thr)), name
        assert math.isnan(S.pair_similarity(cj, ci, thr)), name
    # the diagonal: 1.0, or NaN for no valid gene or a single valid value
    assert S.pair_similarity(cases["m0"][0], cases["m0"][0], 1) == 1.0
    assert math.isnan(S.pair_similarity(np.zeros(5, np.int32), np.zeros(5, np.int32), 1))
    assert math.isnan(S.pair_similarity(np.array([0, 3, 3, 0]), np.array([0, 3, 3, 0]), 1))
    # and an ordinary pair next to them is a number: a = (2, 4, 6, 8), b = (8, 2, 5, 5), m (m + 1)^2 = 100,
    # Sab = 94 - 100, Saa = 120 - 100, Sbb = 118 - 100
    assert S.pair_similarity(np.array([1, 2, 3, 9]), np.array([5, 1, 4, 4]), 1) == -6.0 / math.sqrt(20.0 * 18.0)


def test_gene_distance_restated():
    from scipy.stats import spearmanr
    rng = np.random.default_rng(11)
    mat = rng.normal(size=(6, 15)).round(1)  # (ties)
    np.testing.assert_allclose(S.gene_distance(mat), 1 - spearmanr(mat, axis=1)[0], rtol=0, atol=1e-14)


def _varinfo():
    rng = np.random.default_rng(5)
    return {"mat": rng.normal(size=(12, 8)), "matw": np.ones((12, 8)), "genes": [f"g{i}" for i in range(12)]}


def test_argument_errors():
    from scde_amd import knn, pagoda_gene_cluster_samples, pagoda_gene_clusters, pagoda_gene_clusters_observed
    for bad in ("kendall", "Spearman", "s", None):
        with pytest.raises(ValueError, match="cor_method"):
            pagoda_gene_clusters_observed(_varinfo(), n_clusters=3, cor_method=bad)
        with pytest.raises(ValueError, match="cor_method"):
            pagoda_gene_cluster_samples(12, 8, 0.1, n_clusters=3, n_samples=2, cor_method=bad)
        with pytest.raises(ValueError, match="cor_method"):
            pagoda_gene_clusters(_varinfo(), n_clusters=3, n_samples=2, cor_method=bad)
    counts = golden("knn300.npz")["counts"]
    C = counts.shape[1]
    for shape in ((C, C - 1), (C - 1, C - 1), (C,), (C + 1, C + 1)):
        with pytest.raises(ValueError, match="similarity"):
            knn.knn_model_inputs(counts, similarity=np.zeros(shape), min_size_entries=200)
        with pytest.raises(ValueError, match="similarity"):
            knn.knn_error_models(counts, similarity=np.zeros(shape), min_size_entries=200)
    with pytest.raises(ValueError, match="similarity"):
        knn.knn_model_inputs(counts, similarity=np.eye(C), cor_method="spearman", min_size_entries=200)
    with pytest.raises(ValueError, match="similarity"):
        knn.knn_error_models(counts, similarity=np.eye(C), cor_method="spearman", min_size_entries=200)
    # cor_method = "spearman" alone still raises what tests/test_knn.py pins, now naming the way in
    with pytest.raises(NotImplementedError, match="spearman_cell_similarity"):
        knn.knn_model_inputs(counts, cor_method="spearman")
    with pytest.raises(NotImplementedError, match="spearman_cell_similarity"):
        knn.knn_cell_similarity(counts, cor_method="spearman")


def test_spearman_argument_checks_are_knn_s():
    from scde_amd import knn, rank_columns, spearman_cell_similarity
    counts = golden("knn300.npz")["counts"]
    with pytest.raises(ValueError):
        spearman_cell_similarity(counts.astype(np.float64) + 0.5)
    with pytest.raises(ValueError):
        spearman_cell_similarity(counts, thr=1.5)
    neg = counts.copy()
    neg[3, 4] = -1
    with pytest.raises(ValueError, match="negative"):
        spearman_cell_similarity(neg, thr=0)
    with pytest.raises(ValueError):
        spearman_cell_similarity(np.zeros((3, knn.MAX_CELLS + 1), np.int32))
    with pytest.raises(ValueError):
        spearman_cell_similarity(counts, lds_values=-1)
    with pytest.raises(ValueError):
        rank_columns(np.zeros(5))
