"""Drop-out-adjusted cell-to-cell distances (scde_amd/distance.py, csrc/dist.hip; the reference
vignette's "Adjusted distance measures", vignettes/diffexp.md:231-301).

The reference of every comparison is the numpy restatement below of the formulas in
include/scde_hip.h, evaluated in float64 and in np.longdouble.  A GPU correlation must lie within

    MARGIN x (max |float64 restatement - longdouble restatement| on that case) + FLOOR

of the longdouble value, NaN exactly where the restatement has NaN.  MARGIN = 16: the GPU sums in
4-gene MFMA chains and 32-gene chunks, not in numpy's order, and uses its own exp / log10.
FLOOR = 8 ulp of 1 (1.8e-15) covers cases with so few pairs that the float64 restatement's own
error happens to vanish: the epilogue alone makes about ten roundings of half an ulp each on
quantities of magnitude <= 1.  Measured GPU maxima per test: DESIGN.md section 4.6.

A case is only usable where the restatement itself is well defined: a pair whose exact
correlation is 0/0 (one gene; a constant column) is NaN in one arithmetic and rounding noise in
another unless every operation on it is exact.  The cases below are chosen so that such pairs
are exact (zeros, or dyadic values), and the CPU tests check that the two evaluations agree on
the NaN positions of every case the GPU tests use.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden, gpu_available

MARGIN = 16.0
FLOOR = 8 * 2.0 ** -52
LD = np.longdouble
MODEL_COLUMNS = ["conc.b", "conc.a", "fail.r", "corr.b", "corr.a", "corr.theta", "corr.ltheta.b", "corr.ltheta.t",
                 "corr.ltheta.m", "corr.ltheta.s", "corr.ltheta.r", "conc.a2"]


# ------------------------------------------------------------------ the restatement
def ref_corr(x, y, w):
    """boot::corr over axis 0 (x, y, w broadcast against each other)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        s = w.sum(0)
        m1 = (x * w).sum(0) / s
        m2 = (y * w).sum(0) / s
        return ((x * y * w).sum(0) / s - m1 * m2) / np.sqrt(((x * x * w).sum(0) / s - m1 * m1) *
                                                             ((y * y * w).sum(0) / s - m2 * m2))


def _fail(m, mags, T):
    """scde.failure.probability; mags genes x cells (each cell's own model) -> genes x cells."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = mags * m["conc.a"].astype(T)[None, :]
        if "conc.a2" in m:
            e = e + mags * mags * m["conc.a2"].astype(T)[None, :]
        f = 1 / (np.exp(e + m["conc.b"].astype(T)[None, :]) + 1)
    f[np.isnan(f)] = 0
    return f


def _fpm(m, cd, T):
    with np.errstate(divide="ignore"):
        return (np.log(cd.astype(T)) - m["corr.b"].astype(T)[None, :]) / m["corr.a"].astype(T)[None, :]


def ref_sep(x, u, T):
    """Weights u[g, i] u[g, j]: the columns x columns correlation matrix."""
    x, u = x.astype(T), u.astype(T)
    return ref_corr(x[:, :, None], x[:, None, :], u[:, :, None] * u[:, None, :])


def ref_reciprocal(m, cd, k, T):
    fpm = _fpm(m, cd, T)
    C = cd.shape[1]
    # f1[g, i, j] = f(model_i, fpm[g, j])
    f1 = np.stack([_fail({c: v[[i] * C] for c, v in m.items()}, fpm, T) for i in range(C)], axis=1)
    f2 = f1.transpose(0, 2, 1)
    k = T(k)
    w = np.sqrt((1 - f1) * (1 - f2)) * k + (1 - k)
    x = np.log10(cd.astype(T) + 1)
    return ref_corr(x[:, :, None], x[:, None, :], w)


def ref_jp_modes(jp, prior_x, T):
    with np.errstate(divide="ignore"):
        return np.log(T(10) ** prior_x.astype(T) - 1)[np.argmax(jp, axis=1)]  # the first maximum


def ref_mode(m, cd, modes, jpm, T):
    ps = _fail(m, _fpm(m, cd, T), T)
    pm = _fail(m, np.repeat(jpm.astype(T)[:, None], cd.shape[1], 1), T)
    matw = 1 - np.sqrt(ps * np.sqrt(ps * pm))
    mat = np.log10(np.exp(modes.astype(T)) + 1)
    w = np.sqrt(np.sqrt(matw[:, :, None] * matw[:, None, :]))
    return ref_corr(mat[:, :, None], mat[:, None, :], w)


def ref_keep(m, cd, k, unif):
    """The keep rule on uniforms (cells x genes) -> genes x cells mask (float64 on purpose: it
    is a decision, shared by both evaluations)."""
    q = 1 - _fail(m, _fpm(m, cd, np.float64), np.float64) * k
    u = unif.T
    return np.where(q == 0, False, np.where(q == 1, True, np.where(q <= 0.5, u >= 1 - q, u < q)))


def ref_direct(m, cd, k, unif, T):
    x = np.log10(cd.astype(T) + 1)
    tot = 0
    for s in range(unif.shape[0]):
        keep = ref_keep(m, cd, k, unif[s]).astype(T)
        tot = tot + ref_corr(x[:, :, None], x[:, None, :], keep[:, :, None] * keep[:, None, :])
    return tot / unif.shape[0]


def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def device_uniforms(seed, nsim, ncells, ngenes):
    """The library's generator (include/scde_hip.h): nsim x cells x genes."""
    out = np.empty((nsim, ncells, ngenes))
    ctr = _mix64(np.arange(ngenes * ncells, dtype=np.uint64) + np.uint64(1))
    for s in range(nsim):
        key = _mix64(np.array([(seed + 0x9E3779B97F4A7C15 * (s + 1)) % 2 ** 64], np.uint64))
        out[s] = ((_mix64(key ^ ctr) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(ncells, ngenes)
    return out


# ------------------------------------------------------------------ cases
def _fixture(name, genes=None, cells=None):
    g = golden(name)
    cells = np.arange(g["counts"].shape[1]) if cells is None else np.asarray(cells)
    genes = np.arange(g["counts"].shape[0]) if genes is None else np.asarray(genes)
    mm = g["models"]
    models = {c: mm[cells, j] for j, c in enumerate(MODEL_COLUMNS) if not np.all(np.isnan(mm[:, j]))}
    return g, models, np.ascontiguousarray(g["counts"][genes][:, cells])


def _zero_slice(counts, ncells):
    """(gene, cells): the gene with the most empty cells and the first ncells of them.  One gene
    makes every pair 0/0, which only zeros (x = log10(1) = 0) turn into NaN in every arithmetic."""
    g = int(np.argmax((counts == 0).sum(1)))
    cells = np.nonzero(counts[g] == 0)[0]
    assert cells.size >= ncells, "no gene with enough empty cells for the one-gene slice"
    return np.array([g]), cells[:ncells]


def _recip_cases():
    out = [("esmef500", None, None), ("knn300", None, None)]
    for name in ("esmef500", "knn300"):
        for nc in (1, 2, 17):
            for ng in (1, 5, 65):
                out.append((name, ng, nc))
    return out


def _recip_inputs(name, ng, nc):
    g = golden(name + ".npz")
    if ng is None:
        return _fixture(name + ".npz")[1:]
    genes, cells = _zero_slice(g["counts"], nc) if ng == 1 else (np.arange(7, 7 + ng), np.arange(nc))
    return _fixture(name + ".npz", genes, cells)[1:]


_REF = {}


def _cached(key, fn):
    """(float64, longdouble) evaluations of one case, computed once per session."""
    if key not in _REF:
        _REF[key] = (fn(np.float64), fn(LD))
    return _REF[key]


def _recip_ref(name, ng, nc, k):
    models, cd = _recip_inputs(name, ng, nc)
    return _cached(("recip", name, ng, nc, k), lambda T: ref_reciprocal(models, cd, k, T))


def _gram_inputs(ncells, ngenes):
    rng = np.random.default_rng(1000 * ncells + ngenes)
    if ngenes == 1:  # dyadic values: every pair is exactly 0/0 (module docstring)
        return (rng.integers(8, 33, (1, ncells)) / 8.0, 2.0 ** rng.integers(-1, 2, (1, ncells)))
    return 1.0 + rng.normal(size=(ngenes, ncells)), rng.uniform(0.1, 1.0, (ngenes, ncells))


def _gram_ref(ncells, ngenes):
    x, u = _gram_inputs(ncells, ngenes)
    return _cached(("gram", ncells, ngenes), lambda T: ref_sep(x, u, T))


def _mask_inputs():
    """u in {0, 1}: an all-zero column (3), a constant column where kept (5), two columns that
    share no kept row (6, 7)."""
    rng = np.random.default_rng(77)
    x = 1.0 + rng.normal(size=(70, 20))
    u = (rng.random((70, 20)) < 0.6).astype(np.float64)
    u[:, 3] = 0
    x[:, 5] = 2.0  # a power of two: sum(2 y w) = 2 sum(y w) exactly in any summation order, so 0/0
    u[:, 6] = np.arange(70) % 2
    u[:, 7] = 1 - u[:, 6]
    return x, u


def _direct_inputs():
    _, models, cd = _fixture("esmef500.npz", np.arange(200), None)
    unif = np.random.default_rng(11).random((3, cd.shape[1], cd.shape[0]))
    return models, cd, unif


def _knn_mode_inputs():
    g, models, cd = _fixture("knn300.npz")
    return g, models, cd, np.asfortranarray(g["modes"]), np.ascontiguousarray(g["jp"])


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def assert_close(got, ref, what):
    """got against the (float64, longdouble) restatement pair, module docstring's bound."""
    r64, rld = ref
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert same_nan(r64, rld), f"{what}: the restatement is not well defined on this case"
    nan = np.isnan(rld)
    own = float(np.max(np.abs(r64 - rld)[~nan], initial=0.0))
    err = float(np.max(np.abs(got - rld)[~nan].astype(np.float64), initial=0.0))
    print(f"{what}: gpu max err {err:.3e}, float64 restatement's own {own:.3e}, nan pairs {int(nan.sum())}")
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    assert err <= MARGIN * own + FLOOR, f"{what}: {err:.3e} > {MARGIN} x {own:.3e} + {FLOOR:.3e}"


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("name,ng,nc", _recip_cases())
@pytest.mark.parametrize("k", [0.0, 0.95, 1.0])
def test_restatement_precisions_agree_reciprocal(name, ng, nc, k):
    r64, rld = _recip_ref(name, ng, nc, k)
    assert same_nan(r64, rld)
    ok = ~np.isnan(rld)
    assert np.max(np.abs(r64 - rld)[ok], initial=0.0) < 1e-12
    d = 1 - r64
    assert np.array_equal(d, d.T, equal_nan=True)
    if ng != 1:
        assert np.max(np.abs(np.diag(d))) < 1e-12  # zero diagonal up to rounding
    if ng is None:
        assert ok.all()  # neither fixture yields a NaN pair


def test_restatement_precisions_agree_other_measures():
    for nc in (1, 2, 15, 16, 17, 33):
        for ng in (1, 3, 4, 5, 63, 64, 65, 257):
            r64, rld = _gram_ref(nc, ng)
            assert same_nan(r64, rld) and np.isnan(rld).all() == (ng == 1), (nc, ng)
            assert np.max(np.abs(r64 - rld)[~np.isnan(rld)], initial=0.0) < 1e-11, (nc, ng)
    x, u = _mask_inputs()
    r64, rld = _cached(("mask",), lambda T: ref_sep(x, u, T))
    assert same_nan(r64, rld)
    nan = np.isnan(r64)
    assert nan[3].all() and nan[:, 3].all() and nan[5].all() and nan[:, 5].all() and nan[6, 7] and nan[7, 6]
    assert nan.sum() == 20 * 20 - 18 * 18 + 2
    models, cd, unif = _direct_inputs()
    r64, rld = _cached(("direct",), lambda T: ref_direct(models, cd, 0.9, unif, T))
    assert same_nan(r64, rld) and np.max(np.abs(r64 - rld)[~np.isnan(rld)], initial=0.0) < 1e-12
    g, models, cd, modes, jp = _knn_mode_inputs()
    assert np.isneginf(modes).any()
    r64, rld = _cached(("mode",), lambda T: ref_mode(models, cd, modes, ref_jp_modes(jp, g["prior_x"], T), T))
    assert same_nan(r64, rld) and np.max(np.abs(r64 - rld)[~np.isnan(rld)], initial=0.0) < 1e-12
    d = 1 - r64
    assert np.array_equal(d, d.T, equal_nan=True)


def test_pairwise_complete_restatement_is_pearson():
    """The masked weighted correlation is cor(use = "pairwise.complete.obs")."""
    models, cd, unif = _direct_inputs()
    keep = ref_keep(models, cd, 0.9, unif[0])
    assert 0.2 < keep.mean() < 0.98
    x = np.log10(cd + 1.0)
    r = ref_sep(x, keep.astype(np.float64), np.float64)
    for i, j in ((0, 1), (5, 17), (39, 2)):
        both = keep[:, i] & keep[:, j]
        assert abs(r[i, j] - np.corrcoef(x[both, i], x[both, j])[0, 1]) < 1e-12


def test_device_generator_restatement_is_uniform():
    u = device_uniforms(5, 2, 40, 200)
    assert u.shape == (2, 40, 200) and u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) < 0.01 and abs(u.var() - 1 / 12) < 0.005
    assert not np.array_equal(u[0], u[1]) and not np.array_equal(u, device_uniforms(6, 2, 40, 200))
    # splitmix64's finalizer on its first state from seed 0: the published first output
    assert int(_mix64(np.array([0x9E3779B97F4A7C15], np.uint64))[0]) == 0xE220A8397B1DCDAF


def test_python_argument_checks():
    """Raised before the library (and so the GPU) is touched."""
    from scde_amd import distance
    _, models, cd = _fixture("esmef500.npz", np.arange(10), None)
    for k in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError, match="k must be"):
            distance.reciprocal_distance(models, cd, k=k)
        with pytest.raises(ValueError, match="k must be"):
            distance.direct_dropout_distance(models, cd, k=k)
    with pytest.raises(ValueError, match="n_simulations"):
        distance.direct_dropout_distance(models, cd, n_simulations=0)
    with pytest.raises(ValueError, match="uniforms must have shape"):
        distance.direct_dropout_distance(models, cd, n_simulations=2, uniforms=np.zeros((2, 10, 40)))
    with pytest.raises(ValueError, match="seed"):
        distance.direct_dropout_distance(models, cd, seed=-1)
    with pytest.raises(ValueError, match="number of cells"):
        distance.reciprocal_distance(models, cd[:, :7])
    with pytest.raises(ValueError, match="prior"):
        distance.mode_relative_distance(models, cd)
    with pytest.raises(ValueError, match="posteriors do not match"):
        distance.mode_relative_distance(models, cd, prior={"x": np.linspace(0, 3, 5)},
                                        posteriors={"jp": np.zeros((10, 4)), "modes": np.zeros((10, 40))})
    with pytest.raises(ValueError, match="same shape"):
        distance.weighted_correlation(np.zeros((4, 3)), np.zeros((4, 2)))
    import scde_amd
    for f in ("reciprocal_distance", "mode_relative_distance", "direct_dropout_distance", "weighted_correlation"):
        assert getattr(scde_amd, f) is getattr(distance, f)


def _abi_args():
    _, models, cd = _fixture("esmef500.npz", np.arange(6), np.arange(4))
    from scde_amd.models import model_matrix
    mm, _, sq = model_matrix(models)
    return mm, sq, np.asfortranarray(cd, np.int32), np.zeros((4, 4), order="F")


def test_earg_cases():
    """k outside [0, 1], nsim < 1, ncells < 1 and null outputs are SCDE_EARG (1), checked before
    the device is looked for."""
    from scde_amd import _lib
    from scde_amd.api import _p
    L = _lib.lib()
    mm, sq, cd, out = _abi_args()
    x = np.ones((6, 4), order="F")
    for host in (True, False):  # argument checks come first in the _dev entries too
        rec = L.scde_reciprocal_corr_host if host else L.scde_reciprocal_corr_dev
        dire = L.scde_direct_corr_host if host else L.scde_direct_corr_dev
        mode = L.scde_mode_fail_corr_host if host else L.scde_mode_fail_corr_dev
        sep = L.scde_wcorr_sep_host if host else L.scde_wcorr_sep_dev
        for k in (-0.01, 1.01, float("nan")):
            assert rec(None, _p(cd), 6, 6, 4, _p(mm), sq, k, _p(out)) == 1
            assert b"k must be" in L.scde_last_error()
            assert dire(None, _p(cd), 6, 6, 4, _p(mm), sq, k, 3, None, 1, _p(out)) == 1
        assert dire(None, _p(cd), 6, 6, 4, _p(mm), sq, 0.9, 0, None, 1, _p(out)) == 1
        assert b"nsim" in L.scde_last_error()
        assert rec(None, _p(cd), 6, 6, 0, _p(mm), sq, 0.95, _p(out)) == 1
        assert dire(None, _p(cd), 6, 6, 0, _p(mm), sq, 0.9, 3, None, 1, _p(out)) == 1
        assert mode(None, _p(cd), 6, 6, 0, _p(mm), sq, _p(x), _p(x), _p(out)) == 1
        assert sep(None, _p(x), _p(x), 6, 6, 0, _p(out)) == 1
        assert rec(None, _p(cd), 6, 6, 4, _p(mm), sq, 0.95, None) == 1
        assert dire(None, _p(cd), 6, 6, 4, _p(mm), sq, 0.9, 3, None, 1, None) == 1
        assert mode(None, _p(cd), 6, 6, 4, _p(mm), sq, _p(x), _p(x), None) == 1
        assert sep(None, _p(x), _p(x), 6, 6, 4, None) == 1
        assert b"null" in L.scde_last_error()


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error path")
def test_no_gpu_fails_loudly():
    from scde_amd import _lib, distance
    _, models, cd = _fixture("esmef500.npz", np.arange(10), None)
    g = golden("esmef500.npz")
    with pytest.raises(_lib.ScdeError, match="device"):
        distance.reciprocal_distance(models, cd)
    with pytest.raises(_lib.ScdeError, match="device"):
        distance.direct_dropout_distance(models, cd, n_simulations=2)
    with pytest.raises(_lib.ScdeError, match="device"):
        distance.weighted_correlation(np.ones((3, 2)), np.ones((3, 2)))
    with pytest.raises(_lib.ScdeError, match="device"):
        distance.mode_relative_distance(models, cd, prior={"x": g["prior_x"]},
                                        posteriors={"jp": np.zeros((10, 401)), "modes": np.zeros((10, 40))})
    with pytest.raises(_lib.ScdeError, match="device"):
        distance.mode_relative_distance(models, cd, prior={"x": g["prior_x"], "y": g["prior_y"]})


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("ncells", [1, 2, 15, 16, 17, 33])
def test_gram_kernel(ncells):
    """The 16-cell sub-tile and 32-cell block edges, the MFMA's 4-gene step and the 32-gene
    chunk (63, 64, 65, 257 genes) of k_wcorr_gram."""
    from scde_amd import weighted_correlation
    for ngenes in (1, 3, 4, 5, 63, 64, 65, 257):
        x, u = _gram_inputs(ncells, ngenes)
        got = weighted_correlation(x, u)
        assert_close(got, _gram_ref(ncells, ngenes), f"gram {ncells} cells x {ngenes} genes")
        assert np.array_equal(got, got.T, equal_nan=True)
        assert np.array_equal(got, weighted_correlation(x, u), equal_nan=True)  # bit-repeatable


@pytest.mark.gpu
def test_gram_kernel_masks_and_degenerate_pairs():
    from scde_amd import weighted_correlation
    x, u = _mask_inputs()
    got = weighted_correlation(x, u)
    assert_close(got, _cached(("mask",), lambda T: ref_sep(x, u, T)), "gram 0/1 masks")
    assert np.isnan(got[3]).all() and np.isnan(got[:, 5]).all() and np.isnan(got[6, 7])
    assert np.array_equal(got, weighted_correlation(x, u), equal_nan=True)


@pytest.mark.gpu
def test_gram_kernel_device_entry_and_leading_dimension():
    """scde_wcorr_sep_dev on resident matrices with ld > ngenes gives the host entry's bits."""
    from scde_amd import _lib, api, weighted_correlation
    x, u = _gram_inputs(33, 65)
    want = weighted_correlation(x, u)
    L, ctx = _lib.lib(), api.default_context()
    ld = 70
    bufs = []
    for a in (x, u):
        pad = np.full((ld, 33), np.nan, order="F")
        pad[:65] = a
        p = ctypes.c_void_p()
        _lib.check(L.scde_dev_alloc(ctx.handle, pad.nbytes, ctypes.byref(p)))
        _lib.check(L.scde_h2d(ctx.handle, p, api._p(pad), pad.nbytes))
        bufs.append(p)
    got = np.zeros((33, 33), order="F")
    try:
        _lib.check(L.scde_wcorr_sep_dev(ctx.handle, bufs[0], bufs[1], ld, 65, 33, api._p(got)))
    finally:
        for p in bufs:
            _lib.check(L.scde_dev_free(ctx.handle, p))
    assert np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ng,nc", _recip_cases())
def test_reciprocal(name, ng, nc):
    from scde_amd import reciprocal_distance
    models, cd = _recip_inputs(name, ng, nc)
    for k in (0.0, 0.95, 1.0):
        d = reciprocal_distance(models, cd, k=k)
        assert np.array_equal(d, d.T, equal_nan=True)
        assert (np.diag(d) == 0).all()
        got = 1 - d
        r64, rld = _recip_ref(name, ng, nc, k)
        np.fill_diagonal(got, np.diag(rld).astype(np.float64))  # the API zeroes the distance's diagonal
        assert_close(got, (r64, rld), f"reciprocal {name} {ng}x{nc} k={k}")


@pytest.mark.gpu
def test_reciprocal_diagonal_and_resident_counts():
    """The C entry computes the diagonal by the same formula (1 up to rounding on the
    fixtures); resident counts give the host entry's bits."""
    from scde_amd import _lib, api, reciprocal_distance
    from scde_amd.models import model_matrix
    _, models, cd = _fixture("knn300.npz")
    mm, _, sq = model_matrix(models)
    cdf = np.asfortranarray(cd, np.int32)
    out = np.zeros((64, 64), order="F")
    _lib.check(_lib.lib().scde_reciprocal_corr_host(None, api._p(cdf), 300, 300, 64, api._p(mm), sq, 0.95,
                                                    api._p(out)))
    assert_close(out, _recip_ref("knn300", None, None, 0.95), "reciprocal knn300 C entry")
    assert np.max(np.abs(np.diag(out) - 1)) < 1e-12
    dc = api.DeviceCounts(api.default_context(), cd)
    try:
        d = reciprocal_distance(models, dc)
    finally:
        dc.free()
    assert np.array_equal(d, reciprocal_distance(models, cd))


@pytest.mark.gpu
def test_mode_relative_c_entry():
    """knn300's own modes (with -inf) and jp through scde_mode_fail_corr_host."""
    from scde_amd import _lib, api
    from scde_amd.models import model_matrix
    g, models, cd, modes, jp = _knn_mode_inputs()
    mm, _, sq = model_matrix(models)
    jpm = np.ascontiguousarray(ref_jp_modes(jp, g["prior_x"], np.float64))
    cdf = np.asfortranarray(cd, np.int32)
    out = np.zeros((64, 64), order="F")
    _lib.check(_lib.lib().scde_mode_fail_corr_host(None, api._p(cdf), 300, 300, 64, api._p(mm), sq, api._p(modes),
                                                   api._p(jpm), api._p(out)))
    ref = _cached(("mode",), lambda T: ref_mode(models, cd, modes, ref_jp_modes(jp, g["prior_x"], T), T))
    assert_close(out, ref, "mode-relative knn300")
    assert np.array_equal(out, out.T, equal_nan=True)


@pytest.mark.gpu
def test_mode_relative_python_path():
    """mode_relative_distance end to end (it runs scde_posteriors itself) on 64 genes x 64
    cells, against the restatement on the same call's posterior output."""
    from scde_amd import api, mode_relative_distance
    g, models, cd = _fixture("knn300.npz", np.arange(64), None)
    prior = {"x": g["prior_x"], "y": g["prior_y"]}
    api.set_rand("glibc")
    post = api.scde_posteriors(models, cd, prior, n_randomizations=20, n_cores=1,
                               return_individual_posterior_modes=True)
    d = mode_relative_distance(models, cd, prior=prior, n_randomizations=20, n_cores=1)
    assert np.array_equal(d, mode_relative_distance(models, cd, prior=prior, posteriors=post), equal_nan=True)
    assert (np.diag(d) == 0).all() and np.array_equal(d, d.T, equal_nan=True)
    ref = tuple(ref_mode(models, cd, post["modes"], ref_jp_modes(post["jp"], g["prior_x"], T), T)
                for T in (np.float64, LD))
    got = 1 - d
    np.fill_diagonal(got, np.diag(ref[1]).astype(np.float64))
    assert_close(got, ref, "mode-relative python path")


@pytest.mark.gpu
def test_direct_dropout():
    from scde_amd import direct_dropout_distance
    models, cd, unif = _direct_inputs()
    d = direct_dropout_distance(models, cd, n_simulations=3, k=0.9, uniforms=unif)
    assert (np.diag(d) == 0).all() and np.array_equal(d, d.T, equal_nan=True)
    ref = _cached(("direct",), lambda T: ref_direct(models, cd, 0.9, unif, T))
    got = 1 - d
    np.fill_diagonal(got, np.diag(ref[1]).astype(np.float64))
    assert_close(got, ref, "direct drop-out, caller's uniforms")
    # the device generator: the same bits as its numpy restatement passed as uniforms
    d7 = direct_dropout_distance(models, cd, n_simulations=3, k=0.9, seed=7)
    u7 = device_uniforms(7, 3, cd.shape[1], cd.shape[0])
    assert np.array_equal(d7, direct_dropout_distance(models, cd, n_simulations=3, k=0.9, uniforms=u7),
                          equal_nan=True)
    assert np.array_equal(d7, direct_dropout_distance(models, cd, n_simulations=3, k=0.9, seed=7), equal_nan=True)
    assert not np.array_equal(d7, direct_dropout_distance(models, cd, n_simulations=3, k=0.9, seed=8),
                              equal_nan=True)
    big = 2 ** 64 - 3  # the seed is a full 64-bit key
    assert np.array_equal(direct_dropout_distance(models, cd, n_simulations=1, seed=big),
                          direct_dropout_distance(models, cd, n_simulations=1,
                                                  uniforms=device_uniforms(big, 1, cd.shape[1], cd.shape[0])),
                          equal_nan=True)
