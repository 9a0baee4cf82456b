"""Spearman on the GPU (csrc/spearman.hip) against tests/spearman_ref.py: the rank transform, the
gene clusters' cor_method, the pairwise-complete cell similarity and similarity= of the knn chain.
Ranks and the similarity's sums are exact, so every comparison of them is bit for bit."""
import ctypes
import warnings

import numpy as np
import pytest

import knn_ref as R
import spearman_ref as S
from conftest import golden
from test_gene_cluster_samples import NC, NCLUST, NG, _varinfo
from test_spearman import nan_cases

pytestmark = pytest.mark.gpu

NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ rank transform
def rank_input(nrow, ncol, seed=0):
    """Columns in turn: winsorised (long runs of ties at both bounds), all equal, NaN and +-Inf
    among ordinary values, zeros of both signs among small integers."""
    rng = np.random.default_rng(1000 * nrow + ncol + seed)
    x = np.asfortranarray(rng.normal(size=(nrow, ncol)))
    for j in range(ncol):
        kind = j % 4
        if kind == 0:
            lo, hi = np.quantile(x[:, j], [0.3, 0.7])
            x[:, j] = np.clip(x[:, j], lo, hi)
            x[1::7, j] = 0.0   # (inside the bounds: the quantiles of a normal sample straddle 0)
            x[3::7, j] = -0.0
        elif kind == 1:
            x[:, j] = -3.25
        elif kind == 2:
            x[rng.random(nrow) < 0.2, j] = NAN
            x[rng.random(nrow) < 0.1, j] = np.inf
            x[rng.random(nrow) < 0.1, j] = -np.inf
            x[0, j] = NAN
        else:
            v = rng.integers(-1, 2, nrow).astype(np.float64)
            v[(v == 0) & (rng.random(nrow) < 0.5)] = -0.0
            x[:, j] = v
    return x


def rank_dev(x, in_place):
    """scde_rank_cols_dev on a resident copy of x, into itself or into a second matrix."""
    from scde_amd import api
    from scde_amd._lib import check, lib
    L, ctx = lib(), api.default_context()
    xd, od = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, x.nbytes, ctypes.byref(xd)))
    try:
        check(L.scde_h2d(ctx.handle, xd, api._p(x), x.nbytes))
        if not in_place:
            check(L.scde_dev_alloc(ctx.handle, x.nbytes, ctypes.byref(od)))
        dst = xd if in_place else od
        check(L.scde_rank_cols_dev(ctx.handle, xd, x.shape[0], x.shape[1], dst))
        out, back = np.zeros(x.shape, order="F"), np.zeros(x.shape, order="F")
        check(L.scde_d2h(ctx.handle, api._p(out), dst, x.nbytes))
        check(L.scde_d2h(ctx.handle, api._p(back), xd, x.nbytes))
        if not in_place:
            assert same_bits(back, x)  # the input is left alone
    finally:
        check(L.scde_dev_free(ctx.handle, xd))
        if od:
            check(L.scde_dev_free(ctx.handle, od))
    return out


@pytest.mark.parametrize("nrow,ncol", [(1, 8), (2, 8), (3, 8), (63, 8), (64, 8), (65, 300), (1000, 8), (8193, 3)])
def test_rank_columns(nrow, ncol):
    """8193 rows: the counting path (above the 8192 of the LDS sort)."""
    from scde_amd import rank_columns
    x = rank_input(nrow, ncol)
    ref = S.rank_columns(x)
    got = rank_columns(x)
    assert np.array_equal(np.isnan(got), np.isnan(x))
    assert same_bits(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(ref), 0.0, ref))
    assert same_bits(got[~np.isnan(x)] * 2, np.round(got[~np.isnan(x)] * 2))  # multiples of 0.5
    assert same_bits(got, rank_columns(x))                 # two runs
    assert same_bits(got, rank_dev(x, in_place=False))     # the device entry
    assert same_bits(got, rank_dev(x, in_place=True))      # in place
    for j in (0, 3) if ncol > 3 else (0,):
        zeros = x[:, j] == 0  # both signs
        assert len(set(got[zeros, j])) <= 1 and (nrow < 8 or (np.signbit(x[zeros, j]).any()
                                                               and not np.signbit(x[zeros, j]).all()))
    assert np.all(got[:, 1] == (nrow + 1) / 2)             # the all-equal column


def test_rank_columns_hand_made():
    from scde_amd import rank_columns
    x = np.array([[0.0, 3.0], [-0.0, NAN], [1.0, 1.0], [-1.0, 3.0], [-0.0, NAN], [np.inf, -np.inf], [-np.inf, NAN],
                  [np.inf, 2.0]])
    got = rank_columns(x)
    assert np.array_equal(got[:, 0], [4.0, 4.0, 6.0, 2.0, 4.0, 7.5, 1.0, 7.5])
    assert np.array_equal(got[:, 1], [4.5, NAN, 2.0, 4.5, NAN, 1.0, NAN, 3.0], equal_nan=True)
    assert rank_columns(np.zeros((0, 3))).shape == (0, 3)


# ------------------------------------------------------------------ gene clusters
def same_tree(a, b):
    return (np.array_equal(a.merge, b.merge) and same_bits(a.height, b.height) and np.array_equal(a.order, b.order))


def test_gene_clusters_observed_spearman():
    """The rank kernel is exact and everything after it is the same code: the Spearman call equals
    the Pearson call on host-ranked rows bit for bit.  No batch, so both see the same rows."""
    from scde_amd import pagoda_gene_clusters_observed
    v = _varinfo()
    assert v["mat"].shape == (NG, NC) and v.get("batch") is None
    got = pagoda_gene_clusters_observed(v, cor_method="spearman", trim=0, n_clusters=NCLUST, n_starts=3, seed=5,
                                        return_details=True)
    ranked = dict(v, mat=np.vstack([S.rank(row) for row in v["mat"]]))
    ref = pagoda_gene_clusters_observed(ranked, trim=0, n_clusters=NCLUST, n_starts=3, seed=5, return_details=True)
    assert got["genes"] == ref["genes"] and len(got["genes"]) == NG - 1  # the constant row is dropped by both
    assert same_bits(got["distance"], ref["distance"])
    assert same_tree(got["clustering"], ref["clustering"])
    assert got["clusters"] == ref["clusters"]
    rows = [v["genes"].index(g) for g in got["genes"]]
    # the bar of the Pearson distance (tests/test_hclust.py::test_pagoda_gene_clusters_observed)
    np.testing.assert_allclose(got["distance"], S.gene_distance(v["mat"][rows]), rtol=1e-11, atol=1e-14)
    # only the distance changed: the per-cluster PCA ran on the values, not on the ranks
    for key in got["clusters"]:
        assert not same_bits(got["cl.goc"][key]["xp"]["scores"], ref["cl.goc"][key]["xp"]["scores"]), key
    pear = pagoda_gene_clusters_observed(v, trim=0, n_clusters=NCLUST, n_starts=3, seed=5, return_details=True)
    assert not same_bits(got["distance"], pear["distance"])
    for name in ("p", "pearson"):
        again = pagoda_gene_clusters_observed(v, trim=0, n_clusters=NCLUST, n_starts=3, seed=5, return_details=True,
                                              cor_method=name)
        assert same_bits(again["distance"], pear["distance"]) and same_tree(again["clustering"], pear["clustering"])


@pytest.mark.parametrize("secondary", [False, True])
def test_gene_cluster_samples_spearman(secondary):
    from scde_amd import pagoda_gene_cluster_samples
    rng = np.random.default_rng(77)
    mats = [rng.normal(size=(NG, NC)) for _ in range(2)]
    kw = dict(n_clusters=NCLUST, method="ward.D", secondary_correlation=secondary, return_details=True)
    got = pagoda_gene_cluster_samples(NG, NC, 0, matrices=mats, cor_method="spearman", **kw)
    ranked = [np.vstack([S.rank(row) for row in m]) for m in mats]
    ref = pagoda_gene_cluster_samples(NG, NC, 0, matrices=ranked, **kw)
    pear = pagoda_gene_cluster_samples(NG, NC, 0, matrices=mats, **kw)
    assert np.array_equal(got["n"], ref["n"]) and np.array_equal(got["round"], ref["round"])
    for r in range(2):
        a, b, p = got["details"][r], ref["details"][r], pear["details"][r]
        assert np.array_equal(a["kept"], np.arange(NG)) and np.array_equal(b["kept"], np.arange(NG))
        assert same_bits(a["distance"], b["distance"])
        assert same_tree(a["clustering"], b["clustering"]) and np.array_equal(a["labels"], b["labels"])
        if not secondary:
            np.testing.assert_allclose(a["distance"], S.gene_distance(mats[r]), rtol=1e-11, atol=1e-14)
        # the PC1 variances are those of the values, as in R: the ranks only drive the distance
        assert same_bits(a["matrix"], p["matrix"]) and same_bits(a["matrix"], mats[r])
        assert not same_bits(a["distance"], p["distance"])
    # the default reproduces the Pearson result bit for bit
    for name in ("pearson", "p"):
        again = pagoda_gene_cluster_samples(NG, NC, 0, matrices=mats, cor_method=name, **kw)
        for k in ("n", "var", "round"):
            assert again[k].tobytes() == pear[k].tobytes(), (name, k)
        for r in range(2):
            assert same_bits(again["details"][r]["distance"], pear["details"][r]["distance"])
    if not secondary:
        np.testing.assert_allclose(pear["details"][0]["distance"], 1 - np.corrcoef(mats[0]), rtol=1e-11, atol=1e-14)
    # a round's cluster sizes follow its labels, and its variances are sigma1 of the values in them
    lab = got["details"][0]["labels"]
    assert np.array_equal(got["n"][:NCLUST], np.bincount(lab, minlength=NCLUST + 1)[1:])
    ii = np.flatnonzero(lab == 1)
    s1 = np.linalg.svd(mats[0][ii].T, compute_uv=False)[0] ** 2 / (NC - 1)
    assert got["var"][0] == pytest.approx(s1, rel=1e-9)


# ------------------------------------------------------------------ cell similarity
def synthetic(N, C, seed=0):
    """Poisson-mixture counts with about half zeros; an all-zero cell when there are five."""
    rng = np.random.default_rng(100 * N + C + seed)
    lam = rng.gamma(0.7, 12.0, size=(N, 1)) * rng.uniform(0.4, 2.5, size=(1, C))
    counts = (rng.poisson(lam) * (rng.random((N, C)) < 0.55)).astype(np.int32)
    if C >= 5:
        counts[:, 3] = 0
    return np.asfortranarray(counts)


_ref = {}


def reference(name, counts, thr):
    """The restatement, computed once per (case, thr)."""
    if (name, thr) not in _ref:
        ref = S.cell_similarity(counts, thr)
        ref.setflags(write=False)
        _ref[name, thr] = ref
    return _ref[name, thr]


def check_similarity(name, counts, thr):
    from scde_amd import api, spearman_cell_similarity
    counts = np.asfortranarray(counts, dtype=np.int32)
    ref = reference(name, counts, thr)
    got = spearman_cell_similarity(counts, thr)
    assert same_bits(got, ref), f"{name} thr {thr}: {int((bits(got) != bits(ref)).sum())} entries differ"
    assert same_bits(got, got.T)
    d = np.diag(got)
    nvalid = np.array([len(set(counts[counts[:, c] >= thr, c])) for c in range(counts.shape[1])])
    assert np.all(d[nvalid >= 2] == 1.0) and np.isnan(d[nvalid < 2]).all()
    assert same_bits(got, spearman_cell_similarity(counts, thr, lds_values=8))  # tables in the workspace
    assert same_bits(got, spearman_cell_similarity(counts, thr))                # two runs
    dc = api.DeviceCounts(api.default_context(), counts)
    try:
        assert same_bits(got, spearman_cell_similarity(dc, thr))
        assert same_bits(got, spearman_cell_similarity(dc, thr, lds_values=8))
    finally:
        dc.free()
    return got


@pytest.mark.parametrize("thr", [1, 2, 5])
def test_similarity_on_the_fixture(thr):
    counts = golden("knn300.npz")["counts"]
    got = check_similarity("knn300", counts, thr)
    assert not np.isnan(got[:24, :24]).any()


@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_similarity_shapes(N, C):
    counts = synthetic(N, C)
    for thr in (1, 2):
        check_similarity(f"{N}x{C}", counts, thr)


def test_similarity_more_partners_than_a_block():
    got = check_similarity("40x65", synthetic(40, 65), 1)
    assert np.isfinite(got).sum() > 65 * 32


def test_similarity_leading_dimension():
    from scde_amd import api, spearman_cell_similarity
    from scde_amd._lib import check, lib
    counts = synthetic(65, 5)
    N, C = counts.shape
    big = np.asfortranarray(np.vstack([counts, np.full((9, C), 77, np.int32)]))
    for lds_values in (0, 8):
        sim = np.zeros((C, C), order="F")
        check(lib().scde_spearman_similarity_host(None, api._p(big), N + 9, N, C, 1, lds_values, api._p(sim)))
        assert same_bits(sim, spearman_cell_similarity(counts, 1))
    assert same_bits(sim, reference("65x5", counts, 1))


def test_similarity_all_distinct_large_counts():
    """A cell whose N valid counts are all distinct (D = N), up to 64,402; beside it a cell of few
    distinct values and a cell with no valid gene."""
    rng = np.random.default_rng(3)
    N = 257
    counts = synthetic(N, 4)
    counts[:, 0] = rng.choice(np.arange(1, 64402), N, replace=False)
    counts[7, 0] = 64402
    counts[:, 1] = rng.choice(np.arange(40000, 64000), N, replace=False)
    counts[:, 2] = 0
    assert len(set(counts[:, 0])) == N and counts.max() == 64402 and not (counts[:, 2] >= 1).any()
    for thr in (1, 40000):
        got = check_similarity("distinct", counts, thr)
        assert np.isnan(got[2]).all() and np.isnan(got[:, 2]).all()
    assert np.isfinite(got[0, 1])


@pytest.mark.parametrize("N", [33000, 66000])
def test_similarity_many_genes(N):
    """Above 32768 genes the prepass sorts in its global workspace; above 65535 the codes are 32-bit."""
    counts = synthetic(N, 3)
    counts[:, 2] = np.arange(1, N + 1)  # D = N
    got = check_similarity(f"{N}x3", counts, 1)
    assert np.isfinite(got).all()


def test_similarity_nan_cases():
    for name, (ci, cj, thr) in nan_cases().items():
        counts = np.asfortranarray(np.column_stack([ci, cj, ci + cj + 1]).astype(np.int32))
        got = check_similarity(f"nan-{name}", counts, thr)
        assert np.isnan(got[0, 1]) and np.isnan(got[1, 0]), name
        assert got[2, 2] == 1.0 and got[0, 0] == 1.0, name  # (every case's cell i has two distinct valid values)


def test_similarity_thr_zero():
    counts = synthetic(64, 5)
    got = check_similarity("64x5", counts, 0)
    assert np.isnan(got[3]).all()  # the all-zero cell: every gene valid, all tied
    ok = np.delete(np.arange(5), 3)
    assert np.isfinite(got[np.ix_(ok, ok)]).all()


def test_similarity_stays_resident_for_the_neighbours():
    """scde_knn_neighbours(sim = NULL) finds the Spearman matrix where the Pearson entry leaves its own."""
    from scde_amd import api, spearman_cell_similarity
    from scde_amd._lib import check, lib
    counts = synthetic(65, 5)
    C, k = counts.shape[1], 3
    sim = spearman_cell_similarity(counts, 1)
    nb = np.full((C, k), -7, np.int32)
    check(lib().scde_knn_neighbours(None, None, C, None, k, k, api._p(nb)))
    assert np.array_equal(nb, R.neighbours(sim, k))


def test_similarity_entry_errors():
    from scde_amd import api
    from scde_amd._lib import ScdeError, check, lib
    counts = synthetic(63, 2)
    N = counts.shape[0]
    L = lib()
    msgs = []
    for call in (lambda: L.scde_knn_similarity_host(None, api._p(counts), N, N, 8193, 1, api._p(np.zeros(4))),
                 lambda: L.scde_spearman_similarity_host(None, api._p(counts), N, N, 8193, 1, 0, api._p(np.zeros(4)))):
        with pytest.raises(ScdeError, match="at most 8192") as e:
            check(call())
        msgs.append(str(e.value))
    assert msgs[0].replace("knn_similarity", "spearman_similarity") == msgs[1]
    neg = counts.copy()
    neg[3, 1] = -1
    with pytest.raises(ScdeError, match="negative"):
        check(L.scde_spearman_similarity_host(None, api._p(neg), N, N, 2, 0, 0, api._p(np.zeros((2, 2)))))
    with pytest.raises(ScdeError, match="lds_values"):
        check(L.scde_spearman_similarity_host(None, api._p(counts), N, N, 2, 1, -1, api._p(np.zeros((2, 2)))))


# ------------------------------------------------------------------ the knn chain
def test_model_inputs_with_a_similarity():
    from scde_amd import knn, spearman_cell_similarity
    counts = np.asfortranarray(golden("knn300.npz")["counts"])
    C = counts.shape[1]
    for thr, k in ((1, 5), (2, 16)):
        sim = spearman_cell_similarity(counts, thr)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = knn.knn_model_inputs(counts, similarity=sim, k=k, min_count_threshold=thr, min_size_entries=200)
            pear = knn.knn_model_inputs(counts, k=k, min_count_threshold=thr, min_size_entries=200)
            same = knn.knn_model_inputs(counts, similarity=pear["similarity"], k=k, min_count_threshold=thr,
                                        min_size_entries=200)
        assert same_bits(res["similarity"], sim)
        nb = res["neighbours"]
        assert nb.shape == (C, k) and np.array_equal(nb, R.neighbours(sim, k))
        assert not np.array_equal(nb, pear["neighbours"])  # (the two correlations do order the cells differently)
        fpm, nabove = knn.knn_expected_magnitudes(counts, nb, res["ls"], thr, 0.25)
        assert same_bits(res["fpm"], fpm) and np.array_equal(res["nabove"], nabove)
        # the Pearson similarity handed back in reproduces the default call bit for bit
        for key in ("ls", "similarity", "fpm", "fail_prior"):
            assert same_bits(same[key], pear[key]), key
        for key in ("neighbours", "nabove", "vi"):
            assert np.array_equal(same[key], pear[key]), key
    # groups: NaN between them in the returned matrix, neighbours within them; an asymmetric matrix is taken
    groups = np.arange(C) % 2
    asym = sim + np.triu(np.full((C, C), 1e-3), 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = knn.knn_model_inputs(counts, groups=groups, similarity=asym, k=7, min_size_entries=200)
    cross = groups[:, None] != groups[None, :]
    assert np.isnan(res["similarity"][cross]).all() and same_bits(res["similarity"][~cross], asym[~cross])
    assert np.array_equal(res["neighbours"], R.neighbours(asym, 7, groups))
    assert same_bits(asym, sim + np.triu(np.full((C, C), 1e-3), 1))  # the caller's matrix is not written to


def test_error_models_with_a_similarity():
    from scde_amd import knn, spearman_cell_similarity
    counts = np.asfortranarray(golden("knn300.npz")["counts"])
    sim = spearman_cell_similarity(counts, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = knn.knn_error_models(counts, similarity=sim, k=16, min_size_entries=200)
        ref = knn.knn_error_models(counts, k=16, min_size_entries=200)
    assert len(ref) > 0 and set(ref.index) <= set(got.index)
    assert list(got.columns) == list(ref.columns) and np.isfinite(got["corr.a"].to_numpy()).all()
