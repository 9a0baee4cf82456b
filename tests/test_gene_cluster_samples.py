"""The randomised half of ``pagoda.gene.clusters``: R's rnorm stream on
host and device, the resident winsorize / keep rule / gather, the batched squared largest singular
value (csrc/sigma1.hip), the host statistics (scde_amd/rmt.py) and the two Python entry points.

References.  The stream: a numpy restatement of ``set.seed(i); rnorm()`` (R's seed scrambling
into numpy's MT19937, ``unif_rand`` with its fix-up, the 2^27 combination, ``scipy.stats.norm.ppf``)
and a 40-digit mpmath evaluation ``sqrt(2) erfinv(2 p - 1)`` of the same arguments.  The singular
values: a 40-digit mpmath Rayleigh quotient ``|M v|^2`` at numpy's top right singular vector after
three mpmath power steps -- the quotient's error is the square of the vector's (about 1e-16 over
the relative gap), far below what is measured; the test checks it against ``mpmath.svd_r`` on
small cases.  The tree: tests/test_hclust.py's restatement of the header's contract, repeated
here, applied to the distance the GPU produced, after checking that float64 and longdouble pick
the same merges.

Bars, fixed before any run: for x in {device normal, GPU sigma_1^2} against the 40-digit value,
the error may be at most 16 x the float64 reference's own error on the case (the host function's,
numpy svd's) plus 8 ulp (DESIGN.md section 4.6's form); winsorize, the keep rule, labels, cluster
sizes, row order and the batch-size independence are equalities.

Measured on one MI355X: the device draws' maximum error equals the host function's on every case
(1.45e-15 at most; one value of 4,290 differs from the host's); the worst sigma_1^2 case uses 0.27
of its bar (GPU relative errors up to 6e-16, numpy's own up to 1.6e-15); gumbel_fit's residuals of
the two likelihood equations are 0 and 0 (scipy's 5.6e-16 and 3.3e-16), and the two fits differ by
4.7e-16 (location) and 2.2e-16 (scale).

One check is stated differently from "the float64 and the longdouble keep rule keep the same
genes": on winsorized rounds they cannot, see test_restatement_precisions_agree.
"""
import ctypes

import numpy as np
import pytest

from conftest import gpu_available

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
BIG = 134217728.0


# ------------------------------------------------------------------ restatements
def r_mt(seed):
    """numpy's MT19937 in the state R's set.seed(seed) leaves (Initial scrambling, then
    Randomize's 625 LCG words, dummy[0] = mti = 624)."""
    s = np.uint32(seed)
    with np.errstate(over="ignore"):
        for _ in range(50):
            s = np.uint32(69069) * s + np.uint32(1)
        words = np.empty(625, np.uint32)
        for j in range(625):
            s = np.uint32(69069) * s + np.uint32(1)
            words[j] = s
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": words[1:], "pos": 624}}
    return bg


def r_unif(bg, n):
    x = bg.random_raw(n).astype(np.float64) * 2.3283064365386963e-10
    i2 = 2.328306437080797e-10
    x = np.where(x <= 0.0, 0.5 * i2, x)
    return np.where(1.0 - x <= 0.0, 1.0 - 0.5 * i2, x)


def r_norm_args(seed, n):
    """The n arguments p that norm_rand() hands to qnorm after set.seed(seed)."""
    u = r_unif(r_mt(seed), 2 * n)
    return (np.floor(BIG * u[0::2]) + u[1::2]) / BIG


_CACHE = {}


def _cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


NREF = {1: 10000, 60: 4290}  # draws with a 40-digit reference: the CPU test's 10,000, the GPU cases' 4,290


def ref_normals(seed):
    """(p, scipy ppf, 40-digit value as a float64 and the float64 remainder) of the first
    NREF[seed] draws after set.seed(seed)."""
    def make():
        import mpmath
        from scipy.stats import norm
        p = r_norm_args(seed, NREF[seed])
        with mpmath.workdps(40):
            r2 = mpmath.sqrt(2)
            exact = [r2 * mpmath.erfinv(2 * mpmath.mpf(float(v)) - 1) for v in p]
            hi = np.array([float(v) for v in exact])
            lo = np.array([float(v - mpmath.mpf(float(v))) for v in exact])
        return p, norm.ppf(p), hi, lo
    return _cached(("normals", seed), make)


def err_vs_exact(x, hi, lo):
    """|x - exact| with exact = hi + lo (a double-double)."""
    return np.abs((np.asarray(x) - hi) - lo)


def host_normals(seed, n):
    from scde_amd import _lib, api
    L = _lib.lib()
    st = np.zeros(625, np.uint32)
    out = np.zeros(n)
    _lib.check(L.scde_r_set_seed(seed, api._p(st)))
    _lib.check(L.scde_r_norm_rand(api._p(st), n, api._p(out)))
    return out, st


def restated_matrix(seed, ngenes, ncells, ntr):
    """matrix(rnorm(ngenes * ncells), nrow = ngenes) from the host stream, winsorized (tie-free
    rows: a clip to the order statistics)."""
    m = host_normals(seed, ngenes * ncells)[0].reshape(ncells, ngenes).T.copy()
    if ntr:
        s = np.sort(m, axis=1)
        m = np.clip(m, s[:, [ntr]], s[:, [ncells - ntr - 1]])
    return m


def keep_rule(m, T=LD):
    """which(abs(sum(diff(abs(x)))) > 0): float64 differences, summed in cell order in T."""
    d = np.diff(np.abs(np.asarray(m, np.float64)), axis=1)
    s = np.zeros(d.shape[0], T)
    for k in range(d.shape[1]):
        s = s + d[:, k].astype(T)
    return np.nonzero(s.astype(np.float64) != 0.0)[0]


def ref_steps(d, method, T=np.float64):
    """tests/test_hclust.py's restatement of the hclust contract: raw steps (i, j, h)."""
    d = np.asarray(d)
    n = d.shape[0]
    a = np.full((n, n), np.inf, dtype=T)
    iu = np.triu_indices(n, 1)
    a[iu] = d.T[iu].astype(T)
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
        if method == "ward.D":
            new = ((ni + nk) * dik + (nj + nk) * djk - nk * h) / (ni + nj + nk)
        elif method == "complete":
            new = np.maximum(dik, djk)
        else:
            raise ValueError(method)
        a[lo_i, hi_i] = new
        a[j, :] = np.inf
        a[:, j] = np.inf
        size[i] = ni + nj
    return steps


def r_encode(n, steps):
    label = [-(k + 1) for k in range(n)]
    merge = np.zeros((n - 1, 2), np.int32)
    for s, (i, j, _) in enumerate(steps):
        a, b = label[i], label[j]
        merge[s] = (a, b) if a < 0 and b < 0 else (min(a, b), max(a, b))
        label[i] = s + 1
    return merge, np.array([h for _, _, h in steps], dtype=np.float64)


def ref_tree(d, method):
    """(merge, height) of the float64 restatement, after checking that longdouble picks the same
    pairs (no merge hangs on a rounding)."""
    s64, sld = ref_steps(d, method), ref_steps(d, method, LD)
    assert [(i, j) for i, j, _ in s64] == [(i, j) for i, j, _ in sld], "a merge of this case hangs on a rounding"
    return r_encode(np.asarray(d).shape[0], s64)


class Tree:
    def __init__(self, merge, height):
        self.merge, self.height = merge, height


def sigma1sq_exact(M, div=1):
    """sigma_1(M)^2 / div to far more than double precision, as (hi, lo) doubles."""
    import mpmath
    M = np.asarray(M, np.float64)
    if not M.any():
        return 0.0, 0.0
    v = np.linalg.svd(M, full_matrices=False)[2][0]
    with mpmath.workdps(40):
        rows = [[mpmath.mpf(float(x)) for x in row] for row in M]
        vm = [mpmath.mpf(float(x)) for x in v]
        nc = len(vm)

        def mv(vec):
            return [mpmath.fsum(r[j] * vec[j] for j in range(nc)) for r in rows]
        for _ in range(3):
            w = mv(vm)
            vm = [mpmath.fsum(rows[i][j] * w[i] for i in range(len(rows))) for j in range(nc)]
            nrm = mpmath.sqrt(mpmath.fsum(x * x for x in vm))
            vm = [x / nrm for x in vm]
        w = mv(vm)
        val = mpmath.fsum(x * x for x in w) / div
        hi = float(val)
        return hi, float(val - mpmath.mpf(hi))


def rel_err(x, exact):
    hi, lo = exact
    return abs((x - hi) - lo) / hi if hi else abs(x)


def assert_sigma_bar(got, M, what, worst=None, div=1):
    """|gpu - exact| / exact <= 16 x numpy svd's own relative error on the case + 8 ulp (both
    values divided by div, the variance's n.cells - 1)."""
    exact = sigma1sq_exact(M, div)
    own = rel_err(float(np.linalg.svd(M, compute_uv=False)[0]) ** 2 / div, exact)
    err = rel_err(float(got), exact)
    ratio = err / (16 * own + 8 * EPS)
    print(f"{what}: gpu rel err {err:.3e}, numpy's own {own:.3e}, share of the bar {ratio:.3f}")
    if worst is not None:
        worst.append(ratio)
    assert err <= 16 * own + 8 * EPS, f"{what}: gpu rel err {err:.3e}, numpy's own {own:.3e}"


# pipeline cases: (trim, method, secondary, n_cells); the shape is 120 genes x 24 cells of varinfo
NG, NC, NCLUST, NROUNDS = 120, 24, 6, 3
PIPE_CASES = [(None, "ward.D", False, None), (0, "ward.D", False, None), (None, "complete", False, None),
              (None, "ward.D", True, None), (None, "ward.D", False, 17)]


def _pipe_ntr(trim, ncells):
    t = 3.1 / NC if trim is None else trim
    return t, int(np.floor(ncells * t + 0.5))


# ------------------------------------------------------------------ CPU tests: the stream
def test_norm_rand_textbook_values():
    for seed, want in ((1, [-0.6264538, 0.1836433, -0.8356286]), (42, [1.3709584, -0.5646982, 0.3631284])):
        got = host_normals(seed, 3)[0]
        assert [f"{v:.7f}" for v in got] == [f"{v:.7f}" for v in want], (seed, got)


def test_norm_rand_against_restatement():
    """The first 10,000 draws after set.seed(1): the host function against the 40-digit value,
    within 16 x the numpy restatement's (scipy ppf's) own maximum error + 8 ulp(1)."""
    seed = 1
    p, ppf, hi, lo = ref_normals(seed)
    got = host_normals(seed, NREF[seed])[0]
    own = float(err_vs_exact(ppf, hi, lo).max())
    err = float(err_vs_exact(got, hi, lo).max())
    print(f"seed {seed}, {len(got)} draws: host max err {err:.3e}, restatement's own {own:.3e}, max |host - ppf| "
          f"{np.abs(got - ppf).max():.3e}")
    assert err <= 16 * own + 8 * EPS


def test_norm_rand_advances_the_state_as_two_uniforms():
    from scde_amd import _lib, api
    L = _lib.lib()
    for n in (1, 311, 312, 313, 1000):  # around one refill of the 624 words
        st = host_normals(7, n)[1]
        st2 = np.zeros(625, np.uint32)
        _lib.check(L.scde_r_set_seed(7, api._p(st2)))
        u = np.zeros(2 * n)
        _lib.check(L.scde_r_unif_rand(api._p(st2), 2 * n, api._p(u)))
        assert np.array_equal(st, st2), n
        st3 = np.zeros(625, np.uint32)
        _lib.check(L.scde_r_set_seed(7, api._p(st3)))
        w = np.zeros(2 * n, np.uint32)
        _lib.check(L.scde_r_mt_words(api._p(st3), 2 * n, api._p(w)))
        assert np.array_equal(st, st3)
        assert np.array_equal(w, r_mt(7).random_raw(2 * n).astype(np.uint32))  # numpy's twister, R's seeding
        np.testing.assert_array_equal(u, r_unif(r_mt(7), 2 * n))
    assert L.scde_r_norm_rand(None, 1, api._p(u)) == 1 and L.scde_r_norm_rand(api._p(st), 1, None) == 1


# ------------------------------------------------------------------ CPU tests: rmt.py
def test_wishart_max_par():
    from scde_amd import rmt
    for ndf, pdim in ((24, 1), (24, 20), (1000, 133)):
        a, b = np.sqrt(ndf - 0.5), np.sqrt(pdim - 0.5)
        cen = (a + b) * (a + b) / ndf
        sca = (a + b) * (1 / a + 1 / b) ** (1 / 3) / ndf
        got = rmt.wishart_max_par(ndf, pdim)
        assert got["centering"] == pytest.approx(cen, rel=4 * EPS) and got["scaling"] == pytest.approx(sca, rel=4 * EPS)
    v = rmt.wishart_max_par(24, np.array([1, 20]))
    assert v["centering"].shape == (2,)
    assert v["centering"][1] == rmt.wishart_max_par(24, 20)["centering"]
    assert v["scaling"][0] == rmt.wishart_max_par(24, 1)["scaling"]
    # (24, 1) by hand: sqrt(23.5) = 4.847680, sqrt(.5) = 0.707107: m = 30.85566, centering 1.285652
    assert rmt.wishart_max_par(24, 1)["centering"] == pytest.approx(1.285652, rel=1e-6)
    with pytest.raises(ValueError):
        rmt.wishart_max_par(24, 0)


def _toy_varm():
    rng = np.random.default_rng(5)
    n = rng.integers(1, 40, 30)
    return {"n": n, "var": 1.0 + 0.05 * n + rng.normal(0, 0.1, 30), "round": np.repeat([1, 2, 3], 10)}


def test_score_varm_clvlm_and_tci():
    from scde_amd import rmt
    vm = _toy_varm()
    out, clvlm, tci = rmt.score_varm(vm, 24)
    x = rmt.wishart_max_par(24, vm["n"])
    pm = x["centering"] - 1.2065335745820 * x["scaling"]
    pv = 1.607781034581 * x["scaling"]
    np.testing.assert_array_equal(out["pm"], pm)
    np.testing.assert_array_equal(out["pv"], pv)
    A = np.column_stack([pm, vm["n"].astype(float)])
    coef = np.linalg.lstsq(A, vm["var"], rcond=None)[0]
    assert clvlm["coefficients"]["pm"] == pytest.approx(coef[0], rel=1e-12)
    assert clvlm["coefficients"]["n"] == pytest.approx(coef[1], rel=1e-12)
    np.testing.assert_allclose(clvlm["fitted.values"], A @ coef, rtol=1e-12)
    np.testing.assert_allclose(out["varst"], (vm["var"] - A @ coef) / np.sqrt(pv), rtol=1e-9, atol=1e-12)
    assert list(tci) == [1, 2, 3]
    for r, row in tci.items():
        rows = np.nonzero(vm["round"] == r)[0]
        assert row == rows[np.argmax(out["varst"][rows])]
    # a constructed tie: two rows of one round with the same n and var have the same varst; the first wins
    tie = {k: v.copy() for k, v in vm.items()}
    tie["n"][[13, 17]] = 39
    tie["var"][[13, 17]] = 50.0
    out2, _, tci2 = rmt.score_varm(tie, 24)
    assert out2["varst"][13] == out2["varst"][17] == out2["varst"][10:20].max()
    assert tci2[2] == 13
    with pytest.raises(ValueError, match="rank"):
        rmt.score_varm({"n": np.full(5, 3), "var": np.arange(5.0), "round": np.ones(5, int)}, 24)


def test_gumbel_fit():
    from scipy.stats import gumbel_r

    from scde_amd import rmt
    x = gumbel_r.rvs(loc=0.3, scale=1.7, size=900, random_state=np.random.default_rng(11))
    fit = rmt.gumbel_fit(x)

    def residuals(mu, s):
        """The two likelihood equations, each scaled to O(1): d/dmu and d/dsigma of the mean log-likelihood."""
        z = (x - mu) / s
        e = np.exp(-z)
        return abs(1.0 - e.mean()), abs(np.mean(z * (1.0 - e)) - 1.0)
    mu_s, s_s = gumbel_r.fit(x)
    ours, theirs = residuals(fit["location"], fit["scale"]), residuals(mu_s, s_s)
    dmu, ds = abs(fit["location"] - mu_s), abs(fit["scale"] - s_s)
    msg = f"residuals ours {ours}, scipy {theirs}; |d location| {dmu:.3e}, |d scale| {ds:.3e}"
    print(msg)
    assert ours[0] <= theirs[0] and ours[1] <= theirs[1], msg
    # scipy 1.15 solves the same scale equation with root_scalar(bracket=) = brentq at its defaults,
    # xtol = 2e-12 and rtol = 4 eps: the scale is good to xtol + rtol s, doubled for the two ends;
    # the location follows the scale with slope below 1 + max|x - mu| / s
    tol_s = 2 * (2e-12 + 4 * EPS * s_s)
    tol_mu = (1 + np.abs(x - mu_s).max() / s_s) * tol_s + 16 * EPS * np.abs(x).max()
    assert ds <= tol_s and dmu <= tol_mu, msg
    for bad in ([1.0, 2.0], [3.0] * 20, [1.0, 2.0, np.nan, 4.0]):
        with pytest.raises(ValueError):
            rmt.gumbel_fit(bad)
    # shift and scale equivariance
    f2 = rmt.gumbel_fit(10.0 + 4.0 * x)
    assert f2["location"] == pytest.approx(10.0 + 4.0 * fit["location"], rel=1e-10)
    assert f2["scale"] == pytest.approx(4.0 * fit["scale"], rel=1e-10)


# ------------------------------------------------------------------ CPU tests: preconditions of the GPU cases
@pytest.mark.parametrize("trim,method,secondary,n_cells", PIPE_CASES)
def test_restatement_precisions_agree(trim, method, secondary, n_cells):
    """No GPU case hangs on a rounding: on the restated matrices of every pipeline case the float64
    and longdouble trees make the same merges (on the restated distance; the GPU tests repeat this
    on the GPU's own), and the keep rule's decisions do not depend on the precision of the sum.

    For the keep rule that needs a qualification the winsorized cases force.  A gene whose first
    and last cell were clipped to the same bound has |x[last]| = |x[0]|: its differences telescope
    to zero and their sum is what the 23 roundings of diff() left, a few units of 2^-53 or exactly
    0.  R keeps the gene in the first case and drops it in the second.  About 2 % of the genes of
    a winsorized round are of this kind (3 to 8 of 120 in these cases).  On them a float64
    running sum, which rounds again at every step, is not a restatement of R's long-double sum:
    it disagrees on 1 or 2 genes in every winsorized round here (92 and 109 in round 1).  So the
    float64 and longdouble versions are required to agree on every gene whose ends differ, and on
    the genes whose ends are equal the longdouble sum is held to the exact rational sum instead
    (it agrees on all of them).  Rounds do drop genes (55 in round 2, 26 in round 3), so the gather path runs in the
    ordinary pipeline cases."""
    from fractions import Fraction
    nc = n_cells or NC
    _, ntr = _pipe_ntr(trim, nc)
    for rnd in range(1, NROUNDS + 1):
        m = restated_matrix(rnd, NG, nc, ntr)
        k64, kld = keep_rule(m, np.float64), keep_rule(m, LD)
        ends_equal = np.nonzero(np.abs(m[:, 0]) == np.abs(m[:, -1]))[0]
        differ = np.setxor1d(k64, kld)
        print(f"round {rnd}: ends equal {ends_equal.tolist()}, float64 and longdouble differ on {differ.tolist()}, "
              f"longdouble drops {np.setdiff1d(np.arange(NG), kld).tolist()}")
        assert np.all(np.isin(differ, ends_equal))
        dd = np.diff(np.abs(m), axis=1)
        exact = np.array([g for g in range(NG) if sum(Fraction(float(v)) for v in dd[g]) != 0])
        assert np.array_equal(kld, exact)
        assert len(kld) >= NG - len(ends_equal) and (ntr or len(kld) == NG)
        m = m[kld]
        d = 1 - np.corrcoef(m)
        if secondary:
            d = 1 - np.corrcoef(d)
        np.fill_diagonal(d, 0.0)
        ref_tree(d, method)
    for m in _keep_matrices():
        assert np.array_equal(keep_rule(m, np.float64), keep_rule(m, LD))
        d = 1 - np.corrcoef(m[keep_rule(m)])
        ref_tree(d, "ward.D")


def test_python_argument_checks():
    """Raised before the library (and so the GPU) is touched."""
    import scde_amd
    from scde_amd import cluster
    f = cluster.pagoda_gene_cluster_samples
    with pytest.raises(ValueError, match="at least 2 cells"):
        f(10, 1, 0.1, n_clusters=2)
    with pytest.raises(ValueError, match="at least 2 cells"):
        f(3, 1, 0, n_clusters=2, matrices=[np.ones((3, 1))])
    with pytest.raises(ValueError, match="n_clusters"):
        f(10, 5, 0.1, n_clusters=11)
    with pytest.raises(ValueError, match="unknown method"):
        f(10, 5, 0.1, n_clusters=2, method="centroid")
    with pytest.raises(ValueError, match="10 x 5"):
        f(10, 5, 0.1, n_clusters=2, matrices=[np.ones((5, 10))])
    for name in ("pagoda_gene_cluster_samples", "pagoda_gene_clusters"):
        assert getattr(scde_amd, name) is getattr(cluster, name)


def test_earg_cases():
    """Argument errors of the new C entries are SCDE_EARG (1), before a device is looked for."""
    from scde_amd import _lib
    from scde_amd.api import _p
    L = _lib.lib()
    x = np.zeros(8)
    keep = np.zeros(4, np.int32)
    d = ctypes.c_void_p(x.ctypes.data)  # never dereferenced: every call fails its checks first
    assert L.scde_keep_absdiff_dev(None, d, 1, 4, _p(keep)) == 1 and b"at least 2 cells" in L.scde_last_error()
    assert L.scde_keep_absdiff_dev(None, None, 2, 4, _p(keep)) == 1
    assert L.scde_winsorize_dev(None, d, 2, 4, 0.1, d) == 1 and b"in place" in L.scde_last_error()
    assert L.scde_winsorize_dev(None, d, 8193, 1, 33 / 8193, None) == 1
    y = ctypes.c_void_p(x.ctypes.data + 8)
    assert L.scde_winsorize_dev(None, d, 8193, 1, 33 / 8193, y) == 1 and b"<= 32" in L.scde_last_error()
    assert L.scde_winsorize_dev(None, d, 4, 2, 1.0, y) == 1 and b"out of range" in L.scde_last_error()
    assert L.scde_rnorm_matrix_dev(None, None, 2, 2, d) == 1
    assert L.scde_rnorm_matrix_dev(None, d, 0, 2, d) == 1
    cols = np.array([0, 4], np.int32)
    assert L.scde_gather_cols_dev(None, d, 2, 4, _p(cols), 2, y) == 1 and b"column 1" in L.scde_last_error()
    off = np.array([0, 2, 2], np.int64)
    idx = np.array([0, 1], np.int32)
    out = np.zeros(2)
    assert L.scde_sigma1sq_batch_dev(None, d, 2, 4, 2, _p(off), _p(idx), _p(out)) == 1
    assert b"problem 1 has no columns" in L.scde_last_error()
    off = np.array([0, 1, 2], np.int64)
    idx = np.array([0, 4], np.int32)
    assert L.scde_sigma1sq_batch_dev(None, d, 2, 4, 2, _p(off), _p(idx), _p(out)) == 1
    assert b"problem 1: column index 4" in L.scde_last_error()
    assert L.scde_sigma1sq_batch_dev(None, d, 2, 4, 0, None, None, None) == 0
    assert L.scde_dev_mem_info(None, None, None) == 1


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error path")
def test_no_gpu_fails_loudly():
    from scde_amd import _lib, cluster
    with pytest.raises(_lib.ScdeError, match="device"):
        cluster.pagoda_gene_cluster_samples(10, 5, 0.1, n_clusters=2, n_samples=1)


# ------------------------------------------------------------------ GPU helpers
class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self):
        from scde_amd import _lib, api
        self.L, self.ctx, self.check, self.p = _lib.lib(), api.default_context(), _lib.check, api._p
        self.bufs = []

    def alloc(self, nbytes):
        ptr = ctypes.c_void_p()
        self.check(self.L.scde_dev_alloc(self.ctx.handle, max(nbytes, 8), ctypes.byref(ptr)))
        self.bufs.append(ptr)
        return ptr

    def put(self, a):
        ptr = self.alloc(a.nbytes)
        self.check(self.L.scde_h2d(self.ctx.handle, ptr, self.p(a), a.nbytes))
        return ptr

    def get(self, ptr, shape, dtype=np.float64):
        a = np.zeros(shape, dtype)
        self.check(self.L.scde_d2h(self.ctx.handle, self.p(a), ptr, a.nbytes))
        return a

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for ptr in self.bufs:
            self.check(self.L.scde_dev_free(self.ctx.handle, ptr))


def gpu_sigma1sq(dv, xd, ncells, ngenes, lists):
    off = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    idx = np.ascontiguousarray(np.concatenate(lists).astype(np.int32))
    out = np.full(len(lists), -1.0)
    dv.check(dv.L.scde_sigma1sq_batch_dev(dv.ctx.handle, xd, ncells, ngenes, len(lists), dv.p(off), dv.p(idx),
                                          dv.p(out)))
    return out


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 60])
@pytest.mark.parametrize("ngenes,ncells", [(1, 1), (3, 2), (65, 7), (7, 65), (130, 33)])
def test_draws(ngenes, ncells, seed):
    from scde_amd.cluster import _mt_words
    n = ngenes * ncells
    p, _, hi, lo = ref_normals(seed)
    host = host_normals(seed, n)[0]
    with Dev() as dv:
        words = _mt_words(seed, 2 * n)
        out = dv.alloc(8 * n)
        dv.check(dv.L.scde_rnorm_matrix_dev(dv.ctx.handle, dv.p(words), ngenes, ncells, out))
        got = dv.get(out, (ngenes, ncells))  # gene-contiguous: C order of genes x cells
    flat = got.T.ravel()  # draw t at gene t % ngenes, cell t / ngenes
    own = float(err_vs_exact(host, hi[:n], lo[:n]).max())
    err = float(err_vs_exact(flat, hi[:n], lo[:n]).max())
    print(f"{ngenes} x {ncells} seed {seed}: device max err {err:.3e}, host's own {own:.3e}, "
          f"values differing from the host's: {int((flat != host).sum())}")
    assert err <= 16 * own + 8 * EPS
    if (ngenes, ncells, seed) == (3, 2, 1):
        assert [f"{v:.7f}" for v in got[:, 0]] == ["-0.6264538", "0.1836433", "-0.8356286"]


def _wins_inputs(k, n, ntr):
    """tests/test_gpu_pagoda_edges.py's rows for these shapes: ties at the extremes, +-inf."""
    rng = np.random.default_rng(k * 100000 + n + ntr)
    m = rng.normal(size=(k, n))
    if n >= 200:
        for row, copies in ((0, 40), (1, 20)):
            at = rng.choice(n, size=2 * copies, replace=False)
            m[row, at[:copies]] = m[row].max()
            m[row, at[copies:]] = m[row].min()
        at = rng.choice(n, size=2, replace=False)
        m[1, at[0]], m[1, at[1]] = np.inf, -np.inf
        m[2:, 7] = m[2:, n // 2] = m[2:, n - 3]
    elif n == 2:
        m[0, 1] = m[0, 0]
        m[1] = (np.inf, -np.inf)
    else:
        m[1, 0] = np.inf
        m[2, 0] = -np.inf
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,ntr", [(9, 1, 0), (9, 2, 1), (17, 4097, 5)])
def test_winsorize_dev_equals_winsorizeMatrix(k, n, ntr):
    from scde_amd import pagoda as PG
    m = _wins_inputs(k, n, ntr)
    trim = ntr / n
    assert int(np.floor(n * trim + 0.5)) == ntr
    want = np.asarray(PG.winsorizeMatrix(m, trim))
    with Dev() as dv:
        x = dv.put(np.ascontiguousarray(m))  # genes x cells row-major: a gene's cells contiguous
        out = dv.alloc(m.nbytes)
        dv.check(dv.L.scde_winsorize_dev(dv.ctx.handle, x, n, k, trim, out))
        got = dv.get(out, (k, n))
        assert dv.get(x, (k, n)).tobytes() == m.tobytes()  # the input is left as it was
    np.testing.assert_array_equal(got, want)
    if ntr:
        assert (got != m).any()


def _keep_matrices():
    """Caller matrices for the keep rule: rows whose |x| differences cancel without being
    constant, an alternating-sign row, and rows that stay."""
    rng = np.random.default_rng(77)
    a = rng.normal(size=(9, 3))
    a[2] = [2, 5, -2]   # |x| = 2, 5, 2: differences 3, -3
    a[6] = [1, 2, 4]    # kept
    b = rng.normal(size=(9, 3))
    b[0] = [-3, 0.5, 3]  # dropped
    b[8] = [7, 7, 7]     # constant: dropped too
    return [a, b]


@pytest.mark.gpu
def test_keep_rule_and_gather():
    from scde_amd import pagoda_gene_cluster_samples
    mats = _keep_matrices()
    res = pagoda_gene_cluster_samples(9, 3, 0, n_clusters=3, matrices=mats, return_details=True)
    assert np.array_equal(res["round"], np.repeat([1, 2], 3))
    for r, m in enumerate(mats):
        want = keep_rule(m, LD)
        det = res["details"][r]
        assert np.array_equal(det["kept"], want), (r, det["kept"], want)
        assert len(want) < 9  # the gather path ran
        np.testing.assert_array_equal(det["matrix"], m[want])
        assert res["n"][res["round"] == r + 1].sum() == len(want)
        for c in range(3):
            ii = want[det["labels"] == c + 1]
            assert res["n"][3 * r + c] == len(ii)
            assert_sigma_bar(res["var"][3 * r + c], m[ii].T, f"round {r + 1} cluster {c + 1}", div=2)
    assert 2 not in res["details"][0]["kept"] and 6 in res["details"][0]["kept"]
    # four cells: 1, -1, 1, -1 is dropped although no two neighbours are equal
    rng = np.random.default_rng(78)
    c4 = rng.normal(size=(6, 4))
    c4[3] = [1, -1, 1, -1]
    res = pagoda_gene_cluster_samples(6, 4, 0, n_clusters=2, matrices=[c4], return_details=True)
    assert np.array_equal(res["details"][0]["kept"], [0, 1, 2, 4, 5]) and res["n"].sum() == 5
    with pytest.raises(ValueError, match="at least 2 cells"):
        pagoda_gene_cluster_samples(6, 1, 0, n_clusters=2, matrices=[c4[:, :1]])
    with Dev() as dv:  # the C entry says the same
        x = dv.put(np.ascontiguousarray(c4))
        keep = np.zeros(6, np.int32)
        assert dv.L.scde_keep_absdiff_dev(dv.ctx.handle, x, 1, 6, dv.p(keep)) == 1
        dv.check(dv.L.scde_keep_absdiff_dev(dv.ctx.handle, x, 4, 6, dv.p(keep)))
        assert keep.tolist() == [1, 1, 1, 0, 1, 1]


SIG_CELLS = [1, 2, 3, 17, 64, 65]
SIG_SIZES = [1, 2, 3, 15, 16, 17, 33, 70]
_SIG_WORST = []


@pytest.mark.gpu
@pytest.mark.parametrize("ncells", SIG_CELLS)
def test_sigma1sq_against_mpmath(ncells):
    """Every cluster size against this cell count in one call (both Gram sides: columns <= cells
    and columns > cells), columns drawn in descending and shuffled order."""
    rng = np.random.default_rng(900 + ncells)
    ngenes = 90
    x = rng.normal(size=(ngenes, ncells))  # genes x cells row-major = cells x genes column-major
    lists = []
    for q in SIG_SIZES:
        cols = rng.choice(ngenes, q, replace=False)
        lists.append(np.sort(cols)[::-1] if q % 2 else cols)  # descending for the odd sizes
    with Dev() as dv:
        xd = dv.put(np.ascontiguousarray(x))
        gpu_sigma1sq(dv, xd, ncells, ngenes, lists[::-1])  # a first call leaves another workspace behind
        got = gpu_sigma1sq(dv, xd, ncells, ngenes, lists)
    for q, cols, g in zip(SIG_SIZES, lists, got):
        assert_sigma_bar(g, x[cols].T, f"cells {ncells} columns {q}", _SIG_WORST)
    print(f"worst share of the bar so far: {max(_SIG_WORST):.3f}")


@pytest.mark.gpu
def test_sigma1sq_many_tiles():
    """Several 32 x 32 Gram tiles and many chunks of the summed side, on both sides of the
    columns = cells threshold (sizes the pipeline has at 20,000 genes: clusters of about 130)."""
    rng = np.random.default_rng(4242)
    ncells, ngenes = 130, 320
    x = rng.normal(size=(ngenes, ncells))
    sizes = [129, 130, 131, 300]
    lists = [rng.choice(ngenes, q, replace=False) for q in sizes]
    with Dev() as dv:
        xd = dv.put(np.ascontiguousarray(x))
        gpu_sigma1sq(dv, xd, ncells, ngenes, lists[::-1])
        got = gpu_sigma1sq(dv, xd, ncells, ngenes, lists)
    for q, cols, g in zip(sizes, lists, got):
        assert_sigma_bar(g, x[cols].T, f"cells {ncells} columns {q}")


@pytest.mark.gpu
def test_sigma1sq_special_blocks():
    _check_exact_reference_against_mpmath_svd()  # the reference of every sigma_1^2 comparison here
    rng = np.random.default_rng(17)
    ncells, ngenes = 8, 12
    x = rng.normal(size=(ngenes, ncells))
    u, v = rng.normal(size=ncells), rng.normal(size=5)
    x[0:5] = np.outer(v, u)                      # a rank-one block (to rounding)
    x[5:8] = 0.0                                 # an all-zero block
    x[8] = [2, 0, 0, 0, 0, 0, 0, 0]              # two equal orthogonal dyadic columns
    x[9] = [0, 2, 0, 0, 0, 0, 0, 0]
    lists = [np.arange(5), np.array([7, 5, 6]), np.array([8, 9]), np.array([9, 8]), np.array([4, 3, 2, 1, 0]),
             np.array([5]), np.array([8])]
    with Dev() as dv:
        xd = dv.put(np.ascontiguousarray(x))
        gpu_sigma1sq(dv, xd, ncells, ngenes, [np.arange(12)])
        got = gpu_sigma1sq(dv, xd, ncells, ngenes, lists)
        # more columns than cells: the other Gram side of the same blocks
        wide = np.ascontiguousarray(x[:, :2])
        xw = dv.put(wide)
        gotw = gpu_sigma1sq(dv, xw, 2, ngenes, [np.array([5, 6, 7]), np.array([8, 9, 5]), np.arange(5)])
    assert_sigma_bar(got[0], x[0:5].T, "rank one")
    assert got[1] == 0.0 and got[5] == 0.0
    assert got[2] == 4.0 and got[3] == 4.0 and got[6] == 4.0
    assert_sigma_bar(got[4], x[0:5].T, "rank one, columns descending")
    assert gotw[0] == 0.0 and gotw[1] == 4.0
    assert_sigma_bar(gotw[2], wide[0:5].T, "rank one, cells < columns")
    # non-finite values give NaN, not a hang or an index
    bad = x.copy()
    bad[3, 2] = np.nan
    with Dev() as dv:
        got = gpu_sigma1sq(dv, dv.put(np.ascontiguousarray(bad)), ncells, ngenes, [np.arange(5), np.array([8, 9])])
    assert np.isnan(got[0]) and got[1] == 4.0


def _check_exact_reference_against_mpmath_svd():
    """The Rayleigh-quotient reference agrees with mpmath's own SVD to 1e-30 relative."""
    import mpmath
    rng = np.random.default_rng(3)
    for shape in ((3, 3), (17, 15), (5, 9)):
        M = rng.normal(size=shape)
        hi, lo = sigma1sq_exact(M)
        with mpmath.workdps(40):
            s = mpmath.svd_r(mpmath.matrix(M.tolist()), compute_uv=False)
            top = max(s) ** 2
            assert abs((mpmath.mpf(hi) + mpmath.mpf(lo)) - top) / top < mpmath.mpf(10) ** -30


@pytest.mark.gpu
def test_sigma1sq_batch_equals_single_calls():
    """300 ragged problems in one launch equal, bit for bit, the same problems one per call; the
    compared batch is the second of two calls, so a stale workspace would show."""
    rng = np.random.default_rng(123)
    ncells, ngenes = 17, 200
    x = rng.normal(size=(ngenes, ncells))
    lists = [rng.choice(ngenes, int(q), replace=False) for q in rng.integers(1, 41, 300)]
    with Dev() as dv:
        xd = dv.put(np.ascontiguousarray(x))
        first = gpu_sigma1sq(dv, xd, ncells, ngenes, lists[::-1])
        batch = gpu_sigma1sq(dv, xd, ncells, ngenes, lists)
        single = np.array([gpu_sigma1sq(dv, xd, ncells, ngenes, [v])[0] for v in lists])
    assert batch.tobytes() == single.tobytes()
    assert first[::-1].tobytes() == batch.tobytes()
    ref = np.array([np.linalg.svd(x[v].T, compute_uv=False)[0] ** 2 for v in lists])
    np.testing.assert_allclose(batch, ref, rtol=1e-12)


def _varinfo():
    rng = np.random.default_rng(41)
    load = rng.normal(size=(NG, 3)) * (rng.random((NG, 3)) < 0.4)
    mat = load @ rng.normal(size=(3, NC)) + 0.7 * rng.normal(size=(NG, NC))
    mat[11] = 0.5  # a constant row: dropped by the observed half, counted by the random one
    return {"mat": mat, "matw": rng.uniform(0.1, 1.0, size=(NG, NC)), "genes": [f"g{i}" for i in range(NG)]}


@pytest.mark.gpu
@pytest.mark.parametrize("trim,method,secondary,n_cells", PIPE_CASES)
def test_pipeline(trim, method, secondary, n_cells):
    from scde_amd import cutree, pagoda_gene_cluster_samples
    nc = n_cells or NC
    t, ntr = _pipe_ntr(trim, nc)
    res = pagoda_gene_cluster_samples(NG, nc, t, n_clusters=NCLUST, n_samples=NROUNDS, method=method,
                                      secondary_correlation=secondary, return_details=True)
    assert set(res) == {"n", "var", "round", "details"}
    assert np.array_equal(res["round"], np.repeat(np.arange(1, NROUNDS + 1), NCLUST))
    for rnd in range(1, NROUNDS + 1):
        det = res["details"][rnd - 1]
        m = restated_matrix(rnd, NG, nc, ntr)
        assert np.array_equal(det["kept"], keep_rule(m, LD))  # (winsorized rounds do drop genes: the gather runs)
        m = m[det["kept"]]
        # the device's draws differ from the host's only through qnorm's log and sqrt (2 ulp on
        # r = sqrt(-log p), a rational function of condition below 2 after it): 16 eps relative
        np.testing.assert_allclose(det["matrix"], m, rtol=16 * EPS, atol=0)
        d = 1 - np.corrcoef(m)
        if secondary:
            d = 1 - np.corrcoef(d)
        np.testing.assert_allclose(det["distance"], d, rtol=1e-11, atol=1e-14)  # test_gpu_pagoda.py's matCorr bar
        assert np.all(np.diag(det["distance"]) == 0)
        merge, height = ref_tree(det["distance"], method)
        assert np.array_equal(det["clustering"].merge, merge), f"round {rnd}: merge differs"
        assert np.array_equal(det["clustering"].height, height), f"round {rnd}: heights differ"
        lab = cutree(Tree(merge, height), k=NCLUST)
        assert np.array_equal(det["labels"], lab)
        rows = slice((rnd - 1) * NCLUST, rnd * NCLUST)
        assert np.array_equal(res["n"][rows], np.bincount(lab, minlength=NCLUST + 1)[1:])
        for c in range(NCLUST):
            ii = np.nonzero(lab == c + 1)[0]
            assert_sigma_bar(res["var"][rows][c], m[ii].T, f"round {rnd} cluster {c + 1}", div=max(1, nc - 1))
    if (trim, method, secondary, n_cells) == PIPE_CASES[0]:
        for b in (1, 2, 3):
            again = pagoda_gene_cluster_samples(NG, nc, t, n_clusters=NCLUST, n_samples=NROUNDS, method=method,
                                                rounds_per_batch=b)
            assert set(again) == {"n", "var", "round"}
            for k in again:
                assert again[k].tobytes() == res[k].tobytes(), (b, k)


@pytest.mark.gpu
def test_pagoda_gene_clusters():
    import scde_amd
    from scde_amd import cluster, pagoda_gene_clusters, pagoda_gene_clusters_observed, rmt
    vi = _varinfo()
    res = pagoda_gene_clusters(vi, n_clusters=NCLUST, n_samples=NROUNDS, n_starts=3, seed=5)
    assert set(res) == {"clusters", "xf", "tci", "cl.goc", "varm", "clvlm", "trim"}
    obs = pagoda_gene_clusters_observed(vi, n_clusters=NCLUST, n_starts=3, seed=5)
    assert res["clusters"] == obs["clusters"] and res["trim"] == obs["trim"] == 3.1 / NC
    assert list(res["cl.goc"]) == list(obs["cl.goc"])
    for k in obs["cl.goc"]:
        assert res["cl.goc"][k]["n"] == obs["cl.goc"][k]["n"]
        assert np.array_equal(res["cl.goc"][k]["xp"]["scores"], obs["cl.goc"][k]["xp"]["scores"])
    # the random matrices have nrow(varinfo$mat) genes, the constant row included
    smp = scde_amd.pagoda_gene_cluster_samples(NG, NC, 3.1 / NC, n_clusters=NCLUST, n_samples=NROUNDS)
    for k in ("n", "var", "round"):
        assert np.array_equal(res["varm"][k], smp[k])
    for rnd in range(1, NROUNDS + 1):
        assert res["varm"]["n"][res["varm"]["round"] == rnd].sum() == len(keep_rule(restated_matrix(rnd, NG, NC, 3)))
    scored, clvlm, tci = rmt.score_varm(smp, NC)
    assert res["tci"] == tci and res["clvlm"]["coefficients"] == clvlm["coefficients"]
    assert res["xf"] == rmt.gumbel_fit(scored["varst"])
    # fewer cells in the null model than in varinfo
    r17 = pagoda_gene_clusters(vi, n_clusters=NCLUST, n_samples=2, n_starts=3, seed=5, n_cells=17, old_results=obs)
    s17 = scde_amd.pagoda_gene_cluster_samples(NG, 17, 3.1 / NC, n_clusters=NCLUST, n_samples=2)
    assert np.array_equal(r17["varm"]["var"], s17["var"]) and r17["clusters"] is obs["clusters"]
    # old results with a varm: nothing runs on the device, the given values come back
    calls = []
    real = cluster.pagoda_gene_cluster_samples
    cluster.pagoda_gene_cluster_samples = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        given = {"n": smp["n"].copy(), "var": smp["var"] * 1.5, "round": smp["round"].copy()}
        old = dict(obs, varm=given)
        r2 = pagoda_gene_clusters(vi, n_clusters=NCLUST, n_samples=NROUNDS, old_results=old)
    finally:
        cluster.pagoda_gene_cluster_samples = real
    assert not calls
    assert np.array_equal(r2["varm"]["var"], given["var"]) and np.array_equal(r2["varm"]["n"], given["n"])
    assert r2["clusters"] is obs["clusters"] and r2["cl.goc"] is obs["cl.goc"]
