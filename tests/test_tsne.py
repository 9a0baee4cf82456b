"""CPU tests of the exact t-SNE embedding (scde_amd/embedding.py, csrc/tsne.hip): the numpy
restatement of the contract (tests/tsne_ref.py) is sane on its own, the Python wrapper and the C
entries refuse bad arguments before any device is looked for, and the new symbols are exported.
The kernels are tested in tests/test_gpu_tsne.py."""
import ctypes

import numpy as np
import pytest

import tsne_ref as R

CASES = [(4, 2, 1), (63, 3, 5), (65, 3, 10), (129, 4, 30)]


@pytest.mark.parametrize("n,k,perp", CASES)
def test_restatement_affinities(n, k, perp):
    d, _ = R.clusters(n, k)
    D2 = R.lower_d2(d)
    P, beta, evals, dl = R.affinities(D2, perp)
    assert evals.max() < 200 and (dl < 1e-5).all()
    # every row reaches the perplexity: the entropy of p_.|i recomputed from beta alone
    off = ~np.eye(n, dtype=bool)
    p = np.exp(-beta[:, None] * D2) * off
    s = p.sum(1) + R.DBL_MIN
    H = beta * (D2 * p).sum(1) / s + np.log(s)
    assert np.abs(H - np.log(perp)).max() < 1e-5
    assert np.array_equal(P, P.T)
    assert (np.diag(P) == 0).all() and (P[off] >= 0).all()
    assert abs(P.sum() - 1) < 1e-12
    # another summation order and long double: the same beta, P to rounding
    perm = np.random.default_rng(1).permutation(n)
    for P2, beta2 in (R.affinities(D2, perp, perm=perm)[:2], R.affinities(D2, perp, np.longdouble)[:2]):
        assert np.array_equal(beta2.astype(np.float64), beta)
        assert np.abs(P2 - P).max() <= 1e-14 * P.max()


def test_restatement_reads_the_lower_triangle():
    d, _ = R.clusters(20, 2)
    a = np.where(np.tri(20, k=-1, dtype=bool), d, np.nan)
    assert np.array_equal(R.lower_d2(a), R.lower_d2(d))
    assert np.array_equal(R.lower_d2(d * d, squared=True), (np.tril(d, -1) + np.tril(d, -1).T) ** 2)


def test_restatement_descends_and_switches():
    """The iteration lowers the Kullback-Leibler divergence, keeps Y centred, and the
    exaggeration and momentum switches act after iteration 250, not at it."""
    n = 65
    d, lab = R.clusters(n, 3)
    P = R.affinities(R.lower_d2(d), 10)[0]
    Y0 = 1e-4 * np.random.default_rng(2).normal(size=(n, 2))
    Y, uY, g = R.iterate(P, *R.start(Y0), 0, 250)
    kl0, kl = R.costs(P, Y0).sum(), R.costs(P, Y).sum()
    assert kl < kl0 and np.abs(Y.sum(0)).max() < 1e-9 * np.abs(Y).max()
    at = R.step(P, Y, uY, g, 250)
    assert np.array_equal(at[0], R.step(P, Y, uY, g, 250, stop_lying_iter=250, mom_switch_iter=250)[0])
    assert np.array_equal(at[0], R.step(P, Y, uY, g, 3)[0])
    assert not np.array_equal(at[0], R.step(P, Y, uY, g, 251)[0])
    assert not np.array_equal(R.step(P, Y, uY, g, 251)[0], R.step(P, Y, uY, g, 251, mom_switch_iter=251)[0])
    Yf = R.iterate(P, Y, uY, g, 250, 750)[0]
    assert R.purity(Yf, lab) == 1.0
    perm = np.random.default_rng(3).permutation(n)
    assert np.abs(R.costs(P, Yf, perm=perm) - R.costs(P, Yf)).max() < 1e-12


def test_python_argument_checks():
    """Raised before the library (and so the GPU) is touched."""
    import scde_amd
    from scde_amd import embedding
    d, _ = R.clusters(20, 2)
    for f in (embedding.tsne_embedding, embedding.tsne_affinities):
        with pytest.raises(ValueError, match="at least 4"):
            f(d[:3, :3], perplexity=1)
        with pytest.raises(ValueError, match="perplexity"):
            f(d, perplexity=6.5)  # 3 * 6.5 > 19
        with pytest.raises(ValueError, match="perplexity"):
            f(d, perplexity=0.5)
        with pytest.raises(ValueError, match="perplexity"):
            f(d)  # the default of 30 needs 91 objects
        with pytest.raises(ValueError, match="square"):
            f(d[:, :19], perplexity=5)
        with pytest.raises(ValueError, match="square"):
            f(np.zeros(16), perplexity=1)
        for bad in (np.zeros((19, 2)), np.zeros((20, 3)), np.zeros(40)):
            with pytest.raises(ValueError, match="Y_init"):
                f(d, perplexity=5, Y_init=bad)
        with pytest.raises(TypeError, match="theta"):
            f(d, perplexity=5, theta=0.5)
    with pytest.raises(ValueError, match="max_iter"):
        embedding.tsne_embedding(d, perplexity=5, max_iter=-1)
    for name in ("tsne_embedding", "tsne_affinities", "tsne_iterate", "TsneState"):
        assert getattr(scde_amd, name) is getattr(embedding, name)
    assert "tsne_embedding" in scde_amd.pagoda_cluster_cells.__doc__


def test_exports():
    from scde_amd import _lib
    L = _lib.lib()
    for name in ("scde_tsne_ws_bytes", "scde_tsne_affinities_dev", "scde_tsne_iterate_dev", "scde_tsne_cost_dev",
                 "scde_tsne_host"):
        assert name in _lib.EXPORTS and hasattr(L, name)


def test_seeded_start_is_rnorm():
    """set.seed(1); rnorm(4) is -0.6264538 0.1836433 -0.8356286 1.5952808 in every R since 0.99."""
    from scde_amd.embedding import initial_Y
    y = initial_Y(5, 1)
    assert y.shape == (5, 2)
    assert np.allclose(y.ravel()[:4], 1e-4 * np.array([-0.6264538, 0.1836433, -0.8356286, 1.5952808]), rtol=1e-6)
    assert not np.array_equal(initial_Y(5, 2), y) and np.array_equal(initial_Y(5, 1), y)
    assert np.array_equal(initial_Y(9, 1)[:5], y)


def test_earg_cases():
    """Sizes, perplexity, ld, null pointers, the parameters and the workspace are SCDE_EARG (1),
    checked before the device is looked for."""
    from scde_amd import _lib
    from scde_amd.api import _p
    L = _lib.lib()
    n = 20
    d = np.asfortranarray(R.clusters(n, 2)[0])
    Y, costs, beta = np.zeros((n, 2)), np.zeros(n), np.zeros(n)
    prm = (200.0, 12.0, 250, 250, 0.5, 0.8)

    def host(d_=d, ld=n, n_=n, perp=5.0, prm_=prm, max_iter=10, Y_=Y):
        return L.scde_tsne_host(None, _p(d_), ld, n_, perp, 0, *prm_, max_iter, 1, None, _p(Y_), _p(costs), _p(beta),
                                None)

    assert host(n_=3, perp=1.0) == 1 and b"at least 4" in L.scde_last_error()
    for perp in (6.5, 0.99, float("nan"), float("inf")):
        assert host(perp=perp) == 1 and b"perplexity" in L.scde_last_error()
    assert host(ld=n - 1) == 1 and b"ld" in L.scde_last_error()
    assert host(d_=None) == 1 and host(Y_=None) == 1 and b"null" in L.scde_last_error()
    assert host(max_iter=-1) == 1 and b"negative" in L.scde_last_error()
    assert host(prm_=(float("nan"),) + prm[1:]) == 1 and b"finite" in L.scde_last_error()
    assert not Y.any() and not costs.any() and not beta.any()

    wsb = ctypes.c_int64()
    assert L.scde_tsne_ws_bytes(3, ctypes.byref(wsb)) == 1
    assert L.scde_tsne_ws_bytes(n, None) == 1
    assert L.scde_tsne_ws_bytes(n, ctypes.byref(wsb)) == 0 and wsb.value >= 8 * 5 * n and wsb.value % 256 == 0
    big = ctypes.c_int64()
    assert L.scde_tsne_ws_bytes(20000, ctypes.byref(big)) == 0 and big.value < 8 * 20000 * 20000 // 32
    # host addresses stand in for resident ones: nothing below gets as far as using them
    ws = np.zeros(wsb.value // 8 + 2)
    a16 = ws.ctypes.data % 16 // 8  # the first 16-byte aligned element
    buf = np.zeros(2 * n + 2)
    st = buf[buf.ctypes.data % 16 // 8:][:2 * n]
    P = np.zeros((n, n), order="F")
    aff = L.scde_tsne_affinities_dev
    assert aff(None, _p(d), n, 3, 1.0, 0, _p(P), _p(beta), _p(ws), wsb.value) == 1
    assert aff(None, _p(d), n, n, 6.5, 0, _p(P), _p(beta), _p(ws), wsb.value) == 1
    assert aff(None, _p(d), n - 1, n, 5.0, 0, _p(P), _p(beta), _p(ws), wsb.value) == 1
    assert aff(None, _p(d), n, n, 5.0, 0, None, _p(beta), _p(ws), wsb.value) == 1
    assert aff(None, _p(d), n, n, 5.0, 0, _p(P), _p(beta), None, wsb.value) == 1
    assert b"workspace" in L.scde_last_error()
    assert aff(None, _p(d), n, n, 5.0, 0, _p(P), _p(beta), _p(ws), wsb.value - 1) == 1
    assert b"workspace" in L.scde_last_error()
    it = L.scde_tsne_iterate_dev
    assert it(None, _p(P), 3, *prm, 0, 1, _p(st), _p(st), _p(st), _p(ws[a16:]), wsb.value) == 1
    assert it(None, _p(P), n, *prm, -1, 1, _p(st), _p(st), _p(st), _p(ws[a16:]), wsb.value) == 1
    assert it(None, _p(P), n, *prm, 0, -1, _p(st), _p(st), _p(st), _p(ws[a16:]), wsb.value) == 1
    assert it(None, _p(P), n, *prm, 0, 1, None, _p(st), _p(st), _p(ws[a16:]), wsb.value) == 1
    assert it(None, _p(P), n, *prm, 0, 1, _p(st), _p(st), _p(st), _p(ws[a16:]), 16) == 1
    assert b"workspace" in L.scde_last_error()
    assert it(None, _p(P), n, *prm, 0, 1, _p(st[1:]), _p(st), _p(st), _p(ws[a16:]), wsb.value) == 1
    assert b"16-byte aligned" in L.scde_last_error()
    odd = ctypes.c_void_p(ws.ctypes.data + 8 * a16 + 4)
    assert it(None, _p(P), n, *prm, 0, 1, _p(st), _p(st), _p(st), odd, wsb.value) == 1
    assert b"8-byte aligned" in L.scde_last_error()
    assert aff(None, _p(d), n, n, 5.0, 0, _p(P), _p(beta), odd, wsb.value) == 1
    assert b"8-byte aligned" in L.scde_last_error()
    cost = L.scde_tsne_cost_dev
    assert cost(None, _p(P), 3, _p(st), _p(costs), _p(ws[a16:]), wsb.value) == 1
    assert cost(None, _p(P), n, _p(st), _p(costs), None, wsb.value) == 1
    assert cost(None, _p(P), n, None, _p(costs), _p(ws[a16:]), wsb.value) == 1
    assert not P.any() and not st.any() and not ws.any()
