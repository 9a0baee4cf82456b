"""CPU tests of the neighbourhood stage of knn.error.models: tests/knn_ref.py (the numpy
restatement the GPU tests compare against) on cases worked out by hand, the host statistics of
scde_amd/knn.py against it, and the API's argument errors (raised before the GPU is touched).
"""
import math
import warnings

import numpy as np
import pytest

import knn_ref as R
from conftest import golden

NAN = np.nan


# ------------------------------------------------------------------ TMM and library sizes
def tmm_case(seed=0, rows=400, cols=6):
    rng = np.random.default_rng(seed)
    lam = rng.gamma(0.8, 40.0, size=(rows, 1)) * rng.uniform(0.5, 2.0, size=(1, cols))
    return rng.poisson(lam * rng.lognormal(0, 0.3, size=(rows, cols))).astype(np.float64)


class _Package:
    """scde_amd/knn.py's TMM under the names tests/knn_ref.py gives it, so that every by-hand case
    below pins the shipped code as well as the restatement."""

    def __init__(self):
        from scde_amd import knn
        self.tmm_norm_factors = knn.tmm_norm_factors
        self.tmm_factor = knn._tmm_factor
        self.tmm_reference_column = knn._tmm_reference_column
        self.average_rank = lambda v: knn._average_rank(np.asarray(v, np.float64))
        self.quantile7 = lambda x, p: knn._quantile7(np.asarray(x, np.float64), p)


@pytest.fixture(params=["restatement", "package"])
def T(request):
    return R if request.param == "restatement" else _Package()


def test_tmm_identical_columns_give_ones(T):
    x = np.repeat(tmm_case()[:, :1], 5, axis=1)
    assert np.array_equal(T.tmm_norm_factors(x), np.ones(5))


def test_tmm_scaled_column_changes_nothing(T):
    # identical columns, one of them doubled: obs / nO is the same number bit for bit, every M is
    # exactly 0, so every factor stays 1 before and after the geometric-mean normalisation
    x = np.repeat(tmm_case()[:, :1], 5, axis=1)
    x[:, 2] *= 2
    assert np.array_equal(T.tmm_norm_factors(x), np.ones(5))
    # a general matrix: M, A and so the trimmed rows are unchanged by the doubling (they are
    # functions of obs / nO); only that column's precision weights 1 / v move, so its factor
    # moves a little and the others by the geometric mean alone
    x = tmm_case(1)
    f = T.tmm_norm_factors(x)
    y = x.copy()
    y[:, 2] *= 2
    fy = T.tmm_norm_factors(y)
    assert T.tmm_reference_column(x, x.sum(0)) == T.tmm_reference_column(y, y.sum(0)) != 2
    others = [0, 1, 3, 4, 5]
    np.testing.assert_allclose(fy[others] / fy[0], f[others] / f[0], rtol=1e-13)
    assert abs(fy[2] / fy[0] / (f[2] / f[0]) - 1) < 0.02
    assert np.all(f > 0) and abs(np.exp(np.mean(np.log(f))) - 1) < 1e-14
    assert np.max(np.abs(np.log(f))) > 1e-3  # the case is not trivially all ones


def test_tmm_all_zero_column_has_factor_one(T):
    x = tmm_case(2)
    x[:, 3] = 0
    x = x[np.any(x != 0, axis=1)]  # (the rows TMM drops, so the columns below are the ones it sees)
    lib = x.sum(axis=0)
    with np.errstate(all="ignore"):
        ref = T.tmm_reference_column(x, lib)
        raw = np.array([T.tmm_factor(x[:, j], x[:, ref], lib[j], lib[ref]) for j in range(x.shape[1])])
        f = T.tmm_norm_factors(x)
    # the zero column's quartile is 0 / 0, so it is no column's reference and every M against it is
    # not finite: no row is left and its factor is exactly 1 before the geometric-mean scaling
    assert ref != 3 and raw[3] == 1.0
    others = np.delete(raw, 3)
    assert np.all(np.isfinite(others)) and np.max(np.abs(np.log(others))) > 1e-3
    assert np.array_equal(f, raw / np.exp(np.mean(np.log(raw))))
    assert f[3] == 1.0 / np.exp(np.mean(np.log(raw)))
    # and as the reference of another column: no row is left either
    assert T.tmm_factor(x[:, 0], x[:, 3], lib[0], 0.0) == 1.0


def test_tmm_by_hand(T):
    # one column against a reference column; the row with a zero count drops out (M = -Inf)
    obs = np.array([10.0, 20.0, 30.0, 40.0, 0.0, 50.0, 60.0, 70.0, 80.0, 90.0, 100.0])
    ref = np.array([12.0, 17.0, 33.0, 41.0, 5.0, 47.0, 67.0, 61.0, 89.0, 83.0, 111.0])
    n_o, n_r = obs.sum(), ref.sum()
    keep = obs > 0
    lr = np.log2((obs[keep] / n_o) / (ref[keep] / n_r))
    ae = (np.log2(obs[keep] / n_o) + np.log2(ref[keep] / n_r)) / 2
    v = (n_o - obs[keep]) / n_o / obs[keep] + (n_r - ref[keep]) / n_r / ref[keep]
    n = 10
    lo_l, hi_l = math.floor(n * 0.3) + 1, n - math.floor(n * 0.3)
    lo_s, hi_s = 1, 10
    rl = np.argsort(np.argsort(lr)) + 1  # no ties here
    rs = np.argsort(np.argsort(ae)) + 1
    k = (rl >= lo_l) & (rl <= hi_l) & (rs >= lo_s) & (rs <= hi_s)
    assert len(set(lr)) == 10 and k.sum() == 4
    want = 2.0 ** (np.sum(lr[k] / v[k]) / np.sum(1 / v[k]))
    assert T.tmm_factor(obs, ref, n_o, n_r) == pytest.approx(want, rel=1e-14)
    assert T.tmm_factor(ref, ref, n_r, n_r) == 1.0
    assert T.average_rank(np.array([3.0, 1.0, 3.0, 2.0])).tolist() == [3.5, 1.0, 3.5, 2.0]
    assert T.quantile7([1, 2, 3, 4, 10], 0.75) == 4.0 and T.quantile7([1, 2, 3, 4], 0.75) == 3.25
    # two columns through the whole function: column 0 is the reference (both upper quartiles are
    # equally far from their mean, the first minimum wins), so the factors are 1 and 1 / want
    # before the scaling
    x = np.column_stack([ref, obs])
    assert T.tmm_reference_column(x, x.sum(0)) == 0
    raw = np.array([1.0, want])
    np.testing.assert_allclose(T.tmm_norm_factors(x), raw / np.sqrt(want), rtol=1e-14)


def test_library_size_genes_both_branches():
    C = 4
    counts = np.array([[1, 1, 1, 1],   # 0: everywhere
                       [0, 1, 1, 1],   # 1: three cells
                       [5, 5, 5, 5],   # 2: everywhere
                       [0, 0, 1, 1],   # 3: two
                       [2, 2, 2, 2],   # 4: everywhere
                       [0, 3, 3, 3]])  # 5: three
    # the 4th gene in the order (0, 2, 4, 1, 5, 3) has failures: the first four, ties in gene order
    assert R.library_size_genes(counts, 4, 1).tolist() == [0, 2, 4, 1]
    # the 2nd has none: every gene seen in all cells, however many
    assert R.library_size_genes(counts, 2, 1).tolist() == [0, 2, 4]
    # thr = 2 moves gene 0 out
    assert R.library_size_genes(counts, 2, 2).tolist() == [2, 4]
    with pytest.raises(ValueError):
        R.library_size_genes(counts, 7, 1)
    ls = R.estimate_library_sizes(counts, 2, 1, norm_factors=np.array([1.0, 2.0, 4.0, 2.0]))
    np.testing.assert_allclose(ls, 8 * np.array([0.5, 1.0, 2.0, 1.0]) / 1e6, rtol=1e-15)
    assert C == counts.shape[1]


def test_package_host_statistics_match_the_restatement():
    from scde_amd import knn
    counts = golden("knn300.npz")["counts"]
    for thr in (1, 2):
        assert np.array_equal(knn.library_size_genes(counts, 200, thr), R.library_size_genes(counts, 200, thr))
        a, b = knn.estimate_library_sizes(counts, 200, thr), R.estimate_library_sizes(counts, 200, thr)
        assert np.array_equal(a, b) and np.all(a > 0)
    x = tmm_case(5)
    x[:, 1] = 0
    assert np.array_equal(knn.tmm_norm_factors(x), R.tmm_norm_factors(x))
    v = np.array([2.0, 1.0, 2.0, 2.0, 0.5])
    assert np.array_equal(knn._average_rank(v), R.average_rank(v))
    assert knn.default_k(5) == 2 and knn.default_k(7) == 4 and knn.default_k(6) == 3  # half to even


# ------------------------------------------------------------------ similarity
def test_similarity_one_pass_against_two_pass_and_longdouble():
    counts = golden("knn300.npz")["counts"][:, :20]
    for thr in (1, 2):
        s = R.similarity(counts, thr)
        two = R.similarity_two_pass(counts, thr)
        sl = R.similarity(counts, thr, dtype=np.longdouble)
        assert np.array_equal(np.isnan(s), np.isnan(two))
        assert np.nanmax(np.abs(s - two)) < 1e-13
        assert np.nanmax(np.abs(s - sl.astype(np.float64))) < 1e-13
        np.testing.assert_allclose(np.diag(s), 1.0, rtol=1e-13)


def test_similarity_degenerate_pairs_are_nan():
    counts = np.array([[3, 0, 4], [5, 0, 9], [0, 0, 1], [7, 0, 1]])
    with np.errstate(all="ignore"):
        s = R.similarity(counts, 1)
    assert np.isnan(s[1]).all() and np.isnan(s[:, 1]).all()  # a cell with no valid gene
    assert np.isfinite(s[0, 2]) and s[0, 0] == pytest.approx(1.0)


# ------------------------------------------------------------------ neighbours
def test_neighbour_order_with_ties_and_nan():
    s = np.array([[1.0, 0.5, NAN, 0.5, 0.9, NAN],
                  [0.5, 1.0, 0.2, 0.2, 0.2, 0.2],
                  [NAN, NAN, NAN, NAN, NAN, NAN],
                  [0.5, -0.0, 0.0, 1.0, -1.0, NAN],
                  [0.9, 0.2, 0.3, -1.0, 1.0, 0.3],
                  [NAN, 0.2, NAN, NAN, 0.3, 1.0]])
    nb = R.neighbours(s, 4)
    assert nb.tolist() == [[4, 1, 3, 2],    # 0.9, then the 0.5 tie by index, then the first NaN
                           [0, 2, 3, 4],    # 0.5, then the 0.2 tie by index
                           [0, 1, 3, 4],    # all NaN: index order
                           [0, 1, 2, 4],    # -0 ties with +0: index order; -1 before NaN
                           [0, 2, 5, 1],
                           [4, 1, 0, 2]]
    assert R.neighbours(s, 9).shape == (6, 5)       # k above C - 1 is lowered to C - 1
    assert R.neighbours(s).shape == (6, 3)          # round(6 / 2)
    g = np.array(["a", "b", "a", "a", "b", "a"])
    nbg = R.neighbours(s, 3, g)
    assert nbg.tolist() == [[3, 2, 5], [4, -1, -1], [0, 3, 5], [0, 2, 5], [1, -1, -1], [0, 2, 3]]


# ------------------------------------------------------------------ trimmed mean
def test_trimmed_mean_against_scipy_where_the_definitions_coincide():
    from scipy import stats
    rng = np.random.default_rng(0)
    for n, trim in [(8, 0.25), (10, 0.1), (20, 0.25), (12, 0.0), (5, 0.2), (40, 0.125)]:
        v = rng.gamma(2.0, 3.0, n)
        assert float(n * trim).is_integer()
        assert R.trimmed_mean(v, trim) == pytest.approx(stats.trim_mean(v, trim), rel=1e-14)


def test_trimmed_mean_by_hand():
    v = [5.0, 1.0, 9.0, 3.0, 7.0, 11.0, 2.0]  # sorted 1 2 3 5 7 9 11
    assert R.trimmed_mean(v, 0.25) == (2 + 3 + 5 + 7 + 9) / 5       # floor(1.75) = 1 from each end
    assert R.trimmed_mean(v, 0.3) == (3 + 5 + 7) / 3                 # floor(2.1) = 2
    assert R.trimmed_mean(v, 0.49) == 5.0                            # floor(3.43) = 3: the middle one
    assert R.trimmed_mean(v, 0.5) == 5.0 and R.trimmed_mean(v, 0.9) == 5.0
    assert R.trimmed_mean(v[:6], 0.5) == (5 + 7) / 2                 # 1 3 5 7 9 11: median of an even count
    assert R.trimmed_mean(v[:6], 0.0) == 6.0
    assert R.trimmed_mean([4.0], 0.25) == 4.0 and R.trimmed_mean([4.0, 6.0], 0.25) == 5.0
    assert np.isnan(R.trimmed_mean([], 0.25))
    # the product in double: 10 * 0.3 = 3.0000000000000004 -> 3, 0.1 * 3 ... floor as computed
    assert R.trimmed_mean(np.arange(10.0), 0.3) == np.mean(np.arange(3.0, 7.0))


def test_expected_magnitudes_by_hand():
    counts = np.array([[4, 0, 2, 6, 1],
                       [0, 0, 0, 0, 9],
                       [1, 1, 1, 1, 1]])
    ls = np.array([2.0, 1.0, 0.5, 1.0, 4.0])
    nb = np.array([[1, 2, 3, 4], [0, 2, -1, -1], [0, 1, 3, 4], [4, -1, -1, -1], [0, 1, 2, 3]], np.int32)
    fpm, na = R.expected_magnitudes(counts, nb, ls, thr=1, trim=0.25)
    # gene 0, cell 0: neighbours 1..4 -> valid 2/0.5 = 4, 6/1 = 6, 1/4 = .25 -> n = 3, lo = 1: mean
    assert fpm[0, 0] == (4 + 6 + 0.25) / 3 and na[0, 0] == 2
    assert fpm[0, 1] == (2.0 + 4.0) / 2 and na[0, 1] == 2
    assert np.isnan(fpm[1, 0]) is np.False_ and fpm[1, 0] == 9 / 4 and na[1, 0] == 1
    assert np.isnan(fpm[1, 1]) and na[1, 1] == 0
    assert fpm[2, 3] == 0.25 and na[2, 3] == 0       # 1 is valid (>= 1) and not above (> 1)
    fpm2, na2 = R.expected_magnitudes(counts, nb, ls, thr=2, trim=0.5)
    assert fpm2[0, 0] == (4 + 6) / 2 and na2[0, 0] == 1 and np.isnan(fpm2[2, 0])


def test_valid_genes_and_fail_prior_by_hand():
    tp = 1 - 1e-6
    counts = np.array([[0], [1], [0], [7], [1], [3]])
    fpm = np.array([[2.0], [4.0], [NAN], [5.0], [6.0], [0.0]])
    nabove = np.array([[5], [9], [9], [5], [4], [9]], np.int32)
    vi = R.valid_genes(fpm, nabove, 5, 0)
    assert vi[:, 0].tolist() == [True, True, False, True, False, False]  # NaN, nabove 4, fpm 0 are out
    fp = R.fail_prior(counts, fpm, vi, 1)
    # low genes 0 and 1 (counts <= 1) with fpm 2 and 4: median 3 -> only gene 1 is at or above it
    assert fp[1, 0] == tp and fp[0, 0] == 1 - tp and fp[3, 0] == 1 - tp
    assert (1 - tp) != 1e-6 and np.isnan(fp[[2, 4, 5], 0]).all()
    # no low gene: every entry 1 - tp
    fp = R.fail_prior(np.full((6, 1), 9), fpm, vi, 1)
    assert np.array_equal(fp[vi], np.full(3, 1 - tp))


def test_package_fail_priors_match_the_restatement():
    from scde_amd import knn
    counts = golden("knn300.npz")["counts"]
    ls = R.estimate_library_sizes(counts, 200, 1)
    nb = R.neighbours(R.similarity(counts), 5)
    fpm, na = R.expected_magnitudes(counts, nb, ls)
    vi = R.valid_genes(fpm, na)
    a, b = knn.fail_priors(counts, fpm, vi), R.fail_prior(counts, fpm, vi)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[vi], b[vi])
    assert knn.THRESHOLD_PRIOR == R.TP


# ------------------------------------------------------------------ argument errors
def test_api_argument_errors():
    from scde_amd import knn
    counts = golden("knn300.npz")["counts"]
    C = counts.shape[1]
    with pytest.raises(NotImplementedError):
        knn.knn_cell_similarity(counts, cor_method="spearman")
    with pytest.raises(NotImplementedError):
        knn.knn_model_inputs(counts, cor_method="spearman")
    with pytest.raises(ValueError):
        knn.knn_cell_similarity(counts.astype(np.float64) + 0.5)
    with pytest.raises(ValueError):
        knn.knn_cell_similarity(counts, thr=1.5)
    neg = counts.copy()
    neg[3, 4] = -1
    with pytest.raises(ValueError, match="negative"):
        knn.knn_cell_similarity(neg, thr=0)
    with pytest.raises(ValueError, match="negative"):
        knn.knn_model_inputs(neg, min_size_entries=200)
    with pytest.raises(ValueError):
        knn.knn_cell_similarity(np.zeros((3, knn.MAX_CELLS + 1), np.int32))
    with pytest.raises(ValueError):
        knn.knn_neighbours(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        knn.knn_neighbours(np.zeros((4, 4)), k=0)
    with pytest.raises(ValueError):
        knn.knn_neighbours(np.zeros((4, 4)), k=2, groups=[0, 1, 0])
    nb = np.zeros((C, 3), np.int32)
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb[:5], np.ones(C))
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb, np.ones(C - 1))
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb, -np.ones(C))
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb, np.zeros(C), thr=0)
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb, np.ones(C), trim=-0.1)
    with pytest.raises(ValueError):
        knn.knn_expected_magnitudes(counts, nb, np.ones(C), trim=NAN)
    with pytest.raises(ValueError):
        knn.estimate_library_sizes(counts, min_size_entries=301)
    with pytest.raises(ValueError):
        knn.estimate_library_sizes(counts, 200, norm_factors=np.ones(C - 1))
    with pytest.raises(ValueError):
        knn.knn_model_inputs(counts, min_size_entries=2000)  # fewer genes than min_size_entries
    with pytest.raises(ValueError):
        knn.tmm_norm_factors(np.array([[1.0, -1.0]]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert knn._thr(np.int64(2)) == 2
