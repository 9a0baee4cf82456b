"""CPU checks of the mixture cross-fit of cell pairs: the numpy
restatement (tests/crossfit_ref.py) against its own symmetry and against R's literal list code,
the inputs of scde.fit.models.to.reference, and the arguments.  The kernels are checked against
the restatement in tests/test_gpu_crossfit.py."""
import numpy as np
import pytest

import crossfit_ref as R
from conftest import golden

# Swapping a pair's cells: the largest differences the restatement shows on the six pairs below
# (ES/MEF fixture) are 1.64e-14 in a posterior (absolute), 1.22e-14 in a parameter (relative to
# max(1, |.|)) and 1.2e-16 in llh (relative).  The bounds are ten times those.
SWAP_PAIRS = [(1, 2), (3, 6), (20, 23), (21, 24), (2, 5), (4, 6)]
SWAP_POSTERIOR = 1.64e-13  # measured 1.64e-14
SWAP_PARAMS = 1.22e-13     # measured 1.22e-14
SWAP_LLH = 1.2e-15         # measured 1.2e-16


def swapped_params(p):
    """The parameters of the pair (j, i) as the pair (i, j) states them: component 3 becomes the
    softmax's baseline, the drivers change places."""
    return np.r_[p[0] - p[2], p[1] - p[3], -p[2], -p[3], p[7:10], p[4:7]]


@pytest.mark.parametrize("pair", SWAP_PAIRS)
def test_swapping_the_cells_exchanges_components_1_and_3(pair):
    counts = golden("esmef500.npz")["counts"]
    i, j = pair
    a = R.fit_pair(counts[:, i], counts[:, j])
    b = R.fit_pair(counts[:, j], counts[:, i])
    assert a["status"] == b["status"] == 0 and a["iterations"] == b["iterations"] > 1
    rows = a["rows"]
    np.testing.assert_array_equal(rows, b["rows"])
    dp = np.max(np.abs(a["posterior"][rows] - b["posterior"][rows][:, ::-1]))
    dq = np.max(np.abs(a["params"] - swapped_params(b["params"])) / np.maximum(1.0, np.abs(a["params"])))
    dl = abs(a["llh"] - b["llh"]) / abs(a["llh"])
    print(f"pair {pair}: posterior {dp:.3g}, params {dq:.3g}, llh {dl:.3g}")
    assert dp <= SWAP_POSTERIOR and dq <= SWAP_PARAMS and dl <= SWAP_LLH
    assert np.all(np.isnan(a["posterior"][np.setdiff1d(np.arange(len(counts)), rows)]))


def test_fit_pair_statuses():
    """No rows, a lost component (two identical high-count cells) and a separable concomitant."""
    z = np.zeros(7, np.int32)
    f = R.fit_pair(z, z)
    assert f["status"] == R.NO_ROWS and f["iterations"] == 0 and np.all(f["clusters"] == 0)
    hi = np.arange(50, 90, dtype=np.int32)
    f = R.fit_pair(hi, hi)
    assert f["status"] == R.LOST and f["iterations"] == 1 and np.all(np.isnan(f["params"]))
    counts = golden("esmef500.npz")["counts"]
    f = R.fit_pair(counts[:, 1], counts[:, 13])
    assert f["status"] == R.NOT_FINITE and f["iterations"] == 1


def tiny_crossfit(seed=0):
    """Two groups (cells 0-3 and 4-5), 14 genes, 7 pairs: one failed pair, genes absent from a
    pair (NaN posterior, cluster 0) and rows with cluster 0 (a posterior, cluster 0)."""
    rng = np.random.default_rng(seed)
    N = 14
    counts = rng.integers(0, 30, (N, 6)).astype(np.int32)
    pairs = np.array([[0, 0, 0, 1, 1, 2, 4], [1, 2, 3, 2, 3, 3, 5]], np.int32)
    P = pairs.shape[1]
    cl = rng.integers(1, 4, (N, P)).astype(np.int8)
    cl[:, :3][rng.random((N, 3)) < 0.6] = 2  # (enough genes outside every failure component)
    post = rng.uniform(1e-6, 1 - 1e-6, (2, N, P))
    absent = rng.random((N, P)) < 0.15
    absent[0, 1] = True
    cl[absent] = 0
    post[:, absent] = np.nan
    zero = (rng.random((N, P)) < 0.1) & ~absent
    zero[1, 0] = True
    absent[1, 0] = False
    post[:, 1, 0] = 0.3, 0.6
    cl[zero] = 0
    status = np.zeros(P, np.int32)
    status[3] = 6  # the pair (1, 2) failed
    cl[:, 3] = 0
    post[:, :, 3] = np.nan
    return counts, np.array([0, 0, 0, 0, 1, 1]), {"pairs": pairs, "status": status, "clusters": cl, "posterior": post}


def test_reduction_against_rs_list_code():
    counts, codes, cf = tiny_crossfit()
    ls = np.linspace(0.5, 1.5, 6)
    for mnf in (1, 2, 3):
        lit = R.reduce(counts, codes, cf, ls, mnf, literal=True)
        got = R.reduce(counts, codes, cf, ls, mnf)
        for k in ("vil", "nabove", "vi"):
            np.testing.assert_array_equal(got[k], lit[k], err_msg=k)
        assert 0 < got["vi"].sum() < got["vi"].size and got["vil"].any()
        np.testing.assert_allclose(got["fpm"], lit["fpm"], rtol=1e-14)
        # at most three logs a cell, summed in another order: 3 x 2^-53 relative, and exp's rounding
        np.testing.assert_allclose(got["fail_prior"], lit["fail_prior"], rtol=1e-14)
    # a row of cluster 0 counts in the prior and fails vil; an absent gene does neither
    assert not lit["vil"][1, 0] and not lit["vil"][1, 1] and not lit["vil"][0, 0]
    every = R.reduce(counts, codes, cf, ls, 0)  # (min_nonfailed 0: every gene is valid)
    q = np.array([0.3, cf["posterior"][0, 1, 1], cf["posterior"][0, 1, 2]])
    q = q[~np.isnan(q)]
    np.testing.assert_allclose(every["fail_prior"][1, 0], np.exp(np.mean(np.log(q))), rtol=1e-14)
    # the failed pair (1, 2) takes no part: cell 1 is left with the pairs (0, 1) and (1, 3)
    q = np.array([cf["posterior"][1, 5, 0], cf["posterior"][0, 5, 4]])
    q = q[~np.isnan(q)]
    want = np.exp(np.mean(np.log(q))) if len(q) else 1 - 1e-10
    np.testing.assert_allclose(every["fail_prior"][5, 1], want, rtol=1e-14)


def test_threshold_rule_through_the_reduction():
    """The reduction of the threshold rule's clusters is error_models_ref's closed form: the CPU
    side of the GPU anchor test."""
    import error_models_ref as E
    rng = np.random.default_rng(5)
    counts = (rng.poisson(rng.gamma(0.6, 12.0, (60, 1)) * np.ones((1, 7))) * (rng.random((60, 7)) < 0.7)).astype(np.int32)
    codes = np.array([0, 0, 0, 0, 1, 1, 1])
    pairs = np.array([[0, 0, 0, 1, 1, 2, 4, 4, 5], [1, 2, 3, 2, 3, 3, 5, 6, 6]], np.int32)
    ls = np.linspace(0.7, 1.4, 7)
    cf = R.threshold_crossfit(counts, pairs, 4)
    assert set(np.unique(cf["clusters"])) == {0, 1, 2, 3}
    got = R.reduce(counts, codes, cf, ls, 2)
    ref = E.model_inputs(counts, codes, pairs, ls, 4, 2)
    for k in ("nabove", "vi"):
        np.testing.assert_array_equal(got[k], ref[k])
    np.testing.assert_allclose(got["fpm"], ref["fpm"], rtol=1e-15)
    np.testing.assert_allclose(got["fail_prior"], ref["fail_prior"], rtol=1e-13)


def test_reference_fit_inputs_edges():
    from scde_amd import error_models as EM
    counts = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1], [5, 1, 0]], np.int32)
    ref = np.array([3.0, 1.0, 7.0, 2.0])
    f = ref / ref.sum() * 1e6
    inp = EM.reference_fit_inputs(counts, ref, zero_count_threshold=1, min_fpm=f[3])
    # fpm > min_fpm: the gene that sits on min_fpm is out, as is the smaller one
    np.testing.assert_array_equal(inp["vi"][:, 0], [True, False, True, False])
    np.testing.assert_array_equal(inp["fpm"][[0, 2]], np.repeat(f[[0, 2], None], 3, axis=1))
    assert np.all(np.isnan(inp["fpm"][[1, 3]])) and np.all(np.isnan(inp["fail_prior"][[1, 3]]))
    # count <= zero_count_threshold: a count on the threshold starts in the failure component
    np.testing.assert_array_equal(inp["fail_prior"][[0, 2]], [[1.0, 1.0, 0.0], [0.0, 1.0, 1.0]])
    inp2 = EM.reference_fit_inputs(counts, ref, zero_count_threshold=0, min_fpm=0)
    np.testing.assert_array_equal(inp2["fail_prior"], (counts <= 0).astype(float))
    for bad in (ref[:3], -ref, np.zeros(4), np.array([1.0, np.nan, 1.0, 1.0])):
        with pytest.raises(ValueError, match="reference"):
            EM.reference_fit_inputs(counts, bad)


def test_library_size_genes_with_vil():
    from scde_amd import knn
    counts = np.array([[9, 9, 9], [9, 9, 0], [5, 5, 5], [1, 1, 1]], np.int32)
    np.testing.assert_array_equal(knn.library_size_genes(counts, 2, 4), [0, 2])
    vil = np.array([[1, 0, 0], [1, 1, 1], [0, 0, 0], [1, 1, 1]], np.uint8)
    np.testing.assert_array_equal(knn.library_size_genes(counts, 2, 4, vil=vil), [1, 3])
    np.testing.assert_array_equal(knn.library_size_genes(counts, 3, 4, vil=vil), [1, 3, 0])
    ls = knn.estimate_library_sizes(counts, 2, 4, norm_factors=np.ones(3), vil=vil)
    np.testing.assert_array_equal(ls, counts[[1, 3]].sum(axis=0) / 1e6)
    with pytest.raises(ValueError, match="vil"):
        knn.library_size_genes(counts, 2, 4, vil=vil[:3])


def test_arguments():
    from scde_amd import error_models as EM
    rng = np.random.default_rng(0)
    counts = rng.integers(0, 20, (30, 6)).astype(np.int32)
    with pytest.raises(NotImplementedError, match="crossfit"):
        EM.scde_error_models(counts, threshold_segmentation=False)
    for fn in (EM.scde_error_models, EM.error_model_inputs):
        with pytest.raises(ValueError, match="crossfit must be"):
            fn(counts, crossfit="flexmix")
        with pytest.raises(ValueError, match="crossfit must be"):
            fn(counts, crossfit={"pairs": EM.crossfit_pairs(np.zeros(6, int))})
        with pytest.raises(ValueError, match="min_prior"):
            fn(counts, crossfit="mixture", min_prior=1.0, min_size_entries=10)
        with pytest.raises(ValueError, match="zero_lambda"):
            fn(counts, crossfit="mixture", zero_lambda=0.0, min_size_entries=10)
        with pytest.raises(ValueError, match="crossfit_iter"):
            fn(counts, crossfit="mixture", crossfit_iter=0, min_size_entries=10)
        with pytest.raises(NotImplementedError):
            fn(counts, crossfit="mixture", min_count_threshold=0)
    pairs = EM.crossfit_pairs(np.zeros(6, int))
    P = pairs.shape[1]
    good = {"pairs": pairs, "status": np.zeros(P, np.int32), "clusters": np.full((30, P), 2, np.int8),
            "posterior": np.full((2, 30, P), 0.5)}
    with pytest.raises(ValueError, match="does not belong"):
        EM.error_model_inputs(counts, crossfit=dict(good, clusters=good["clusters"][:29]), min_size_entries=10)
    with pytest.raises(ValueError, match="codes 0 to 3"):
        EM.error_model_inputs(counts, crossfit=dict(good, clusters=good["clusters"] + 2), min_size_entries=10)
    with pytest.raises(ValueError, match="differs"):
        EM.error_model_inputs(counts, crossfit=good, pairs=pairs[:, ::-1], min_size_entries=10)
    failed = dict(good, status=np.where((pairs[0] == 2) | (pairs[1] == 2), 6, 0).astype(np.int32))
    with pytest.warns(UserWarning, match="cross-fit of cells"), pytest.raises(ValueError, match="pair of cell 2 failed"):
        EM.error_model_inputs(counts, crossfit=failed, min_size_entries=10)
    with pytest.raises(ValueError, match="min_prior"):
        EM.crossfit_models(counts, min_prior=-0.1)
    with pytest.raises(ValueError, match="iter"):
        EM.crossfit_models(counts, iter=0)
    with pytest.raises(ValueError, match="two different cells"):
        EM.crossfit_models(counts, pairs=np.array([[0], [0]]))
    with pytest.raises(ValueError, match="negative"):
        EM.crossfit_models(counts, min_count_threshold=-1)
    with pytest.raises(ValueError, match="reference"):
        EM.scde_fit_models_to_reference(counts, np.ones(29))
