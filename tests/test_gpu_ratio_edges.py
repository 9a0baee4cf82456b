"""The ratio-posterior and summary kernel (k_ratio_summary, scde_amd/csrc/ratio.hip) on the GPU at the
value-dependent edges of tests/ratio_edge_cases.py, behind its three entries (scde_matSlideMult,
scde_ratio_summary, scde_distribution_summary) and the batch-corrected DE path, against the oracle.

matSlideMult is compared bit for bit (every NaN equal to every NaN; the signs of zeros and infinities
checked); the normalised ratio by its NaN mask and assert_posterior_close(rel=1e-12), the bar of
test_gpu_parity.test_ratio_and_summary; lb / mle / ub / ce exactly and Z by assert_z_close.  The one
group compared otherwise is Z at zi = m - 1 (test_last_column_quirk).  What the cases are
and why the oracle is right on them: tests/test_ratio_edges.py."""
import numpy as np
import pytest

import ratio_edge_cases as E
from conftest import assert_cz_close, assert_posterior_close, assert_z_close, golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from scde_amd import api as A
    A.set_rand("glibc")
    return A


def assert_same_bits(got, ref, what, names=None):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nan = np.isnan(got) & np.isnan(ref)
    bad = ~nan & ((got != ref) | (np.signbit(got) != np.signbit(ref)))
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        row = f" (row '{names[idx[0]]}')" if names is not None else ""
        raise AssertionError(f"{what}: {int(bad.sum())} entries differ in {int(bad.any(axis=-1).sum())} rows; first at "
                             f"{idx}{row}: {got[idx]!r} vs {ref[idx]!r}")


def c_ratio_summary(api, A, B, y, diffv, zi):
    """scde_ratio_summary with both outputs: (ratio, res)."""
    from scde_amd._lib import check, lib
    a, b = api._f64(A), api._f64(B)
    nr, n = a.shape
    y = None if y is None else np.ascontiguousarray(y, np.float64)
    dv = np.ascontiguousarray(diffv, np.float64)
    ratio = np.zeros((nr, 2 * n - 1), order="F")
    res = np.zeros((nr, 5), order="F")
    check(lib().scde_ratio_summary(api._p(a), api._p(b), nr, n, api._p(y), api._p(dv), int(zi), api._p(ratio),
                                   api._p(res)))
    return ratio, res


def c_summary(api, X, diffv, zi):
    from scde_amd._lib import check, lib
    x = api._f64(X)
    nr, m = x.shape
    dv = np.ascontiguousarray(diffv, np.float64)
    res = np.zeros((nr, 5), order="F")
    check(lib().scde_distribution_summary(api._p(x), nr, m, api._p(dv), int(zi), api._p(res)))
    return res


def oracle_summary(oracle, X, diffv, zi):
    ref = oracle.quick_distribution_summary(X, diffv, diffv[zi] * E.LOG2_10)
    return np.column_stack([ref[k] for k in ("lb", "mle", "ub", "ce", "Z")])


def check_summary(got, ref, what, names=None):
    for j, k in enumerate(("lb", "mle", "ub", "ce")):
        assert_same_bits(got[:, j], ref[:, j], f"{what} {k}", names)
    assert_z_close(got[:, 4], ref[:, 4], what=f"{what} Z")


# ------------------------------------------------------------------ A. matSlideMult on sparse and odd rows
@pytest.mark.parametrize("n", E.SLIDE_SIZES)
def test_slide_bit_exact(api, oracle, n):
    A, B, names, _ = E.slide_rows(n)
    assert_same_bits(api.matSlideMult(A, B), oracle.matSlideMult(A, B), f"matSlideMult n = {n}", names)


@pytest.mark.parametrize("skip_prior", [False, True], ids=["prior", "skip-prior"])
@pytest.mark.parametrize("n", E.SLIDE_SIZES)
def test_slide_ratio_posterior(api, oracle, n, skip_prior):
    A, B, names, _ = E.slide_rows(n)
    prior = E.slide_prior(n)
    with np.errstate(all="ignore"):  # (the column names of a one-point grid are 0 / 0)
        got = api.calculate_ratio_posterior(A, B, prior, skip_prior_adjustment=skip_prior).values
    ref = oracle.calculate_ratio_posterior(A, B, prior["y"], skip_prior_adjustment=skip_prior)
    bad = np.isnan(got) != np.isnan(ref)
    assert not bad.any(), (f"n = {n}: NaN mask differs in rows " +
                           ", ".join(f"'{names[r]}'" for r in np.nonzero(bad.any(1))[0][:8]))
    assert_posterior_close(got, ref, rel=1e-12, what=f"ratio n = {n}")


# ------------------------------------------------------------------ B. more rows than workgroups
def test_more_rows_than_workgroups(api, oracle):
    A, B, y, diffv, zi = E.many_rows()
    assert_same_bits(api.matSlideMult(A, B), oracle.matSlideMult(A, B), "matSlideMult, 65,666 rows")
    ratio, res = c_ratio_summary(api, A, B, y, diffv, zi)
    ref_ratio = oracle.calculate_ratio_posterior(A, B, y)
    assert_same_bits(ratio, ref_ratio, "ratio, 65,666 rows")
    assert api.expectation_column(diffv, 0.0) == zi
    check_summary(res, oracle_summary(oracle, ref_ratio, diffv, zi), "65,666 rows")


# ------------------------------------------------------------------ C. the summary
@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_summary_rows(api, oracle, m):
    """Thresholds met exactly, one ulp away and through quarter-ulp terms; bounds not found; ties."""
    names, X = E.summary_rows(m)
    diffv = E.summary_diffv(m)
    zi = (m - 1) // 2
    check_summary(c_summary(api, X, diffv, zi), oracle_summary(oracle, X, diffv, zi), f"m = {m}", names)


@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_z_all_mass_on_one_column(api, oracle, m):
    diffv = E.summary_diffv(m)
    for zi in E.z_columns(m):
        rows = E.onehot_rows(m, zi)
        X = np.asfortranarray(np.vstack([x for _, x in rows]))
        assert api.expectation_column(diffv, diffv[zi] * E.LOG2_10) == zi
        check_summary(c_summary(api, X, diffv, zi), oracle_summary(oracle, X, diffv, zi), f"m = {m} zi = {zi}",
                      [n for n, _ in rows])


@pytest.mark.parametrize("m", [5, 129, 801])
def test_last_column_quirk(api, oracle, m):
    """zi = m - 1: gs + zv is 1 up to rounding and qnorm(p > 1) is NaN, in R itself; the kernel's
    double-double sum may round the other way.  Each Z is NaN or the zl branch's value."""
    X = E.last_column_rows(m)
    diffv = E.summary_diffv(m)
    zi = m - 1
    assert api.expectation_column(diffv, diffv[zi] * E.LOG2_10) == zi
    got = c_summary(api, X, diffv, zi)
    ref = oracle_summary(oracle, X, diffv, zi)
    for j, k in enumerate(("lb", "mle", "ub", "ce")):
        assert_same_bits(got[:, j], ref[:, j], f"m = {m} zi = m - 1 {k}")
    zl = np.array([min(oracle.qnorm(E.oracle_gs(x, zi), False), 0.0) for x in X])
    z = got[:, 4]
    print(f"m = {m}, zi = m - 1: Z is NaN on {np.isnan(z).sum()} rows, the oracle's on {np.isnan(ref[:, 4]).sum()}, "
          f"{(np.isnan(z) != np.isnan(ref[:, 4])).sum()} of {len(z)} differ in NaN-ness")
    fin = ~np.isnan(z)
    if fin.any():
        assert_z_close(z[fin], zl[fin], what=f"m = {m} zi = m - 1 Z against the zl branch")


@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_fused_equals_separate(api, oracle, m):
    """scde_ratio_summary's res against scde_distribution_summary of the ratio the same call returned
    (bit for bit), and against the oracle's summary of that ratio."""
    A, B, y = E.ratio_inputs(m)
    diffv = E.summary_diffv(m)
    for zi in sorted({0, (m - 1) // 2}):
        for py in (y, None):
            ratio, res = c_ratio_summary(api, A, B, py, diffv, zi)
            assert ratio.shape[1] == m
            assert_same_bits(c_summary(api, ratio, diffv, zi), res, f"m = {m} zi = {zi}: separate against fused")
            ref = oracle.calculate_ratio_posterior(A, B, y, skip_prior_adjustment=py is None)
            assert_posterior_close(ratio, ref, rel=1e-12, what=f"ratio m = {m}")
            check_summary(res, oracle_summary(oracle, ratio, diffv, zi), f"m = {m} zi = {zi} fused")


def test_summary_refusals(api, oracle):
    from scde_amd._lib import ScdeError
    X = np.asfortranarray(np.full((2, 4), 0.25))
    with pytest.raises(ScdeError):
        c_summary(api, X, np.arange(4.0), 1)  # m even
    names, X = E.summary_rows(5)
    diffv = E.summary_diffv(5)
    for zi in (-1, 5):
        with pytest.raises(ScdeError, match="zi"):
            c_summary(api, X, diffv, zi)
        with pytest.raises(ScdeError, match="zi"):
            c_ratio_summary(api, np.ones((2, 3)), np.ones((2, 3)), None, diffv, zi)
    check_summary(c_summary(api, X, diffv, 2), oracle_summary(oracle, X, diffv, 2), "after the refusals", names)


# ------------------------------------------------------------------ D. the LDS bound
def _n_limits(api):
    ctx = api.default_context()
    return int(ctx.stat("ratio_n_lds64")), int(ctx.stat("ratio_n_max"))


def _three_rows(n):
    rng = np.random.default_rng(n)
    A = rng.random((3, n))
    B = rng.random((3, n)) ** 3
    A[1, : n // 3] = 0.0
    A[1, n // 2:: 2] = 0.0
    B[1, n - n // 5:] = 0.0
    A[2, 5] = np.inf
    return np.asfortranarray(A), np.asfortranarray(B)


@pytest.mark.parametrize("which", ["last-within-64KiB", "first-above-64KiB", "1401", "largest"])
def test_slide_at_lds_sizes(api, oracle, which):
    lds64, nmax = _n_limits(api)
    assert 401 < lds64 < 1401 < nmax
    n = {"last-within-64KiB": lds64, "first-above-64KiB": lds64 + 1, "1401": 1401, "largest": nmax}[which]
    A, B = _three_rows(n)
    assert_same_bits(api.matSlideMult(A, B), oracle.matSlideMult(A, B), f"matSlideMult n = {n}")


def _models(g, oracle):
    return {c: g["models"][:, j] for j, c in enumerate(oracle.MODEL_COLUMNS) if not np.all(np.isnan(g["models"][:, j]))}


def _batch_labels():
    return np.array(["b1" if (i * 5) % 3 else "b2" for i in range(40)])


def test_n_above_the_largest_is_refused(api, oracle):
    from scde_amd._lib import ScdeError
    lds64, nmax = _n_limits(api)
    n = nmax + 1
    says = rf"at most n = {nmax}\b"
    ones = np.ones((1, n))
    with pytest.raises(ScdeError, match=says):
        api.matSlideMult(ones, ones)
    with pytest.raises(ScdeError, match=says):
        c_ratio_summary(api, ones, ones, None, np.zeros(2 * n - 1), 0)
    with pytest.raises(ScdeError, match=says):
        c_summary(api, np.ones((1, 2 * n - 1)), np.zeros(2 * n - 1), 0)
    g = golden("esmef500.npz")
    models, counts = _models(g, oracle), np.ascontiguousarray(g["counts"][:4])
    flat = lambda G: {"x": np.linspace(0.0, 5.0, G), "y": np.full(G, 1.0 / G)}  # noqa: E731
    with pytest.raises(ScdeError, match=says):
        api.scde_expression_difference(models, counts, flat(n), groups=list(g["groups"]), n_randomizations=2)
    with pytest.raises(ScdeError, match=says):
        api.scde_expression_difference(models, counts, flat((nmax + 1) // 2 + 1), groups=list(g["groups"]),
                                       batch=_batch_labels(), n_randomizations=2)
    A, B, names, _ = E.slide_rows(33)
    assert_same_bits(api.matSlideMult(A, B), oracle.matSlideMult(A, B), "matSlideMult after the refusals", names)


def test_batch_corrected_length_out_700(api, oracle):
    """length_out = 700 is a grid of G = 701 points; the batch-corrected path's third ratio pass runs
    over the 2 G - 1 = 1401 columns of the first two: above 64 KiB of LDS."""
    from scde_amd.prior import expression_prior
    g = golden("esmef500.npz")
    lds64, nmax = _n_limits(api)
    models = _models(g, oracle)
    counts = np.ascontiguousarray(g["counts"][:30])
    prior = expression_prior(models, counts, length_out=700)
    assert lds64 < 2 * len(prior["x"]) - 1 <= nmax
    batch = _batch_labels()
    api.set_rand("glibc")
    out = api.scde_expression_difference(models, counts, prior, groups=list(g["groups"]), batch=batch,
                                         n_randomizations=10, n_cores=2, return_posteriors=True)
    ref = oracle.scde_expression_difference_batch(models, counts, prior["x"], prior["y"], g["groups"], list(batch),
                                                  n_randomizations=10, n_cores=2, return_posteriors=True)
    for i in range(2):
        assert_posterior_close(out["joint.posteriors"][i], ref["joint.posteriors"][i], what=f"jp{i}")
    assert_posterior_close(out["difference.posterior"].values, ref["difference.posterior"], what="ratio")
    assert_posterior_close(out["batch.adjusted.difference.posterior"].values,
                           ref["batch.adjusted.difference.posterior"], what="batch-adjusted ratio")
    for table in ("batch.effect", "results", "batch.adjusted"):
        got, want = out[table], ref[table]
        for k in ("lb", "mle", "ub", "ce"):
            np.testing.assert_array_equal(got[k].to_numpy(), want[k], err_msg=f"{table}.{k}")
        assert_z_close(got["Z"].to_numpy(), want["Z"], what=f"{table}.Z")
        assert_cz_close(got["cZ"].to_numpy(), want["cZ"], got["Z"].to_numpy(), want["Z"], what=f"{table}.cZ")
