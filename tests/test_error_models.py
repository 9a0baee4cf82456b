"""scde.error.models without a GPU: the numpy restatements of tests/error_models_ref.py (the
contract of DESIGN.md section 4.16) against each other and against R, the pair enumeration, and
the argument checks of scde_amd/error_models.py.

R's own stored result of scde.error.models on the ES/MEF data (``o.ifm``, the ``models`` of
tests/golden/esmef_vignette_inputs.npz) is the yardstick of the fit: if the restatement does not
reproduce it, the contract was misread.  Over all 40 cells the restatement measured (median, 90th
percentile, worst; printed by test_restatement_reproduces_r_on_all_40_cells):

    |d conc.b|              1.10e-4   6.70e-4   5.07e-3
    |d conc.a|              1.79e-5   1.60e-4   8.55e-4
    |d corr.b|              4.05e-9   3.42e-6   1.34e-5
    |d corr.a|              6.22e-10  5.14e-7   2.07e-6
    |d corr.theta| / theta  1.25e-9   3.53e-7   7.04e-7
    fail.r                  equal

corr.theta is reproduced like the other columns.  conc.* are nnet's early stop against the exact
maximiser (DESIGN.md section 4.15 has the same finding for knn.error.models).
"""
import itertools
import math

import numpy as np
import pytest

import error_models_ref as E
from conftest import golden

#: what the restatement measured against R's 40 stored rows, last digit rounded up: median, 90th
#: percentile, worst cell (absolute; corr.theta relative).  tests/test_gpu_error_models.py takes
#: its bounds against R from this table.
ESMEF_RESTATEMENT = {"conc.b": (1.11e-4, 6.70e-4, 5.08e-3), "conc.a": (1.79e-5, 1.61e-4, 8.56e-4),
                     "corr.b": (4.06e-9, 3.43e-6, 1.34e-5), "corr.a": (6.22e-10, 5.15e-7, 2.07e-6),
                     "corr.theta": (1.25e-9, 3.53e-7, 7.05e-7)}
COLUMN = {"conc.b": 0, "conc.a": 1, "corr.b": 3, "corr.a": 4, "corr.theta": 5}


def distances_to_r(rows, ref):
    """Per column of ESMEF_RESTATEMENT: (median, 90th percentile, worst) over the cells."""
    out = {}
    for name, c in COLUMN.items():
        d = np.abs(rows[:, c] - ref[:, c])
        if name == "corr.theta":
            d = d / np.abs(ref[:, c])
        out[name] = (float(np.median(d)), float(np.quantile(d, 0.9)), float(d.max()))
    return out


# ------------------------------------------------------------------ the input stage
def small_counts(N, C, seed, zero=0.55):
    rng = np.random.default_rng(seed)
    lam = rng.gamma(0.6, 12.0, size=(N, 1)) * rng.uniform(0.5, 2.0, size=(1, C))
    return (rng.poisson(lam) * (rng.random((N, C)) > zero)).astype(np.int32)


def all_pairs(codes):
    out = []
    for g in np.unique(codes):
        out += E.combn_pairs([int(c) for c in np.flatnonzero(codes == g)])
    return np.array(out, dtype=np.int64).T.reshape(2, -1)


def same_inputs(a, b):
    np.testing.assert_array_equal(a["vi"], b["vi"])
    np.testing.assert_array_equal(a["nabove"], b["nabove"])
    np.testing.assert_array_equal(np.isnan(a["fpm"]), np.isnan(b["fpm"]))
    np.testing.assert_array_equal(np.isnan(a["fail_prior"]), ~a["vi"])
    np.testing.assert_array_equal(np.isnan(b["fail_prior"]), ~b["vi"])
    v = a["vi"]
    np.testing.assert_allclose(a["fpm"][v], b["fpm"][v], rtol=1e-14, atol=0)
    np.testing.assert_allclose(a["fail_prior"][v], b["fail_prior"][v], rtol=1e-13, atol=0)


@pytest.mark.parametrize("thr", [1, 4])
@pytest.mark.parametrize("thin", [False, True])
def test_literal_lists_reduce_to_the_closed_forms(thr, thin):
    """R's per-pair lists (vi, clusters, posterior) and its %in% / rowMeans(log(.), na.rm) give
    vil = counts >= thr, nabove, vi, the plain mean and the counted geometric mean: groups of 2,
    3 and 7 cells, all pairs and a thinned list that leaves a cell with a single pair."""
    codes = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2])
    counts = small_counts(90, 12, 3 + thr)
    counts[:, 5] = 0  # a cell without a read ...
    counts[:40, 9] = 0  # ... and rows where its only partner of the thinned list has none either
    pairs = all_pairs(codes)
    if thin:
        keep = np.ones(pairs.shape[1], bool)
        g7 = np.flatnonzero(codes[pairs[0]] == 2)
        keep[g7[1::2]] = False
        keep[(pairs[0] == 5) | (pairs[1] == 5)] = False
        keep[np.flatnonzero((pairs[0] == 5) & (pairs[1] == 9))] = True
        pairs = pairs[:, keep]
    ls = np.random.default_rng(1).uniform(0.5, 2.0, 12)
    for mnf in (1, 3):
        lit = E.model_inputs(counts, codes, pairs, ls, thr, mnf, literal=True)
        clo = E.model_inputs(counts, codes, pairs, ls, thr, mnf)
        same_inputs(lit, clo)
    # vil itself, for the group of 7
    ids = [int(c) for c in np.flatnonzero(codes == 2)]
    gp = [(int(a), int(b)) for a, b in pairs.T if codes[a] == 2]
    vil = E.literal_inputs(counts, ids, gp, ls, thr, 3)["vil"]
    np.testing.assert_array_equal(vil, counts[:, ids] >= thr)
    if thin:  # the cell whose every partner row is both-zero on genes the other cells make valid: R's nai rows
        v = clo["vi"][:40, 5]
        assert v.any() and np.all(clo["fail_prior"][:40, 5][v] == 1 - 1e-10)
    # the min over the group size is real: in the group of two, one other cell is enough
    assert np.array_equal(clo["vi"][:, 0], counts[:, 1] >= thr)


def test_fail_prior_levels():
    """One pair: high where the cell is below the threshold and its partner is not."""
    counts = np.array([[0, 9], [9, 0], [9, 9], [0, 0], [2, 2], [2, 9]], np.int32)
    r = E.model_inputs(counts, np.zeros(2, int), np.array([[0], [1]]), np.ones(2), 4, 0)
    hi, lo = 1 - 1e-6, 1 - (1 - 1e-6)  # threshold.prior and 1 - threshold.prior, as doubles
    np.testing.assert_allclose(r["fail_prior"][:, 0], [hi, lo, lo, 1 - 1e-10, lo, hi], rtol=1e-14)
    np.testing.assert_allclose(r["fail_prior"][:, 1], [lo, hi, lo, 1 - 1e-10, lo, lo], rtol=1e-14)
    np.testing.assert_allclose(r["fpm"][:, 0], counts[:, 1])


def test_fpm_does_not_cancel():
    """A cell holding a million reads beside cells holding one: the others' mean is exact."""
    counts = np.ones((4, 5), np.int32)
    counts[:, 2] = 1000000
    r = E.model_inputs(counts, np.zeros(5, int), all_pairs(np.zeros(5, int)), np.full(5, 3.0), 1, 3)
    np.testing.assert_allclose(r["fpm"][:, 2], 1 / 3.0, rtol=4 * 5 * 2.0 ** -52)
    np.testing.assert_allclose(r["fpm"][:, 0], (3 / 3.0 + 1000000 / 3.0) / 4, rtol=4 * 5 * 2.0 ** -52)


# ------------------------------------------------------------------ the pairs
def test_pairs_come_in_combn_order_group_by_group():
    from scde_amd import error_models as EM
    groups = np.array(["b", "a", "b", "a", "b", "a", "a"])
    p = EM.crossfit_pairs(groups)
    a, b = [1, 3, 5, 6], [0, 2, 4]
    want = list(itertools.combinations(a, 2)) + list(itertools.combinations(b, 2))  # R's levels: "a" first
    assert [tuple(x) for x in p.T] == want
    assert EM.crossfit_pairs(None, ncells=4).shape == (2, 6)
    with pytest.raises(ValueError, match="single cell"):
        EM.crossfit_pairs(np.array([0, 0, 1]))


def test_sampled_pairs():
    """The sampled form (not checked against R): no more than max_pairs + cells * min_pairs_per_cell
    distinct pairs, at least min_pairs_per_cell of them for every cell, the same for the same
    seed, and only for the group that needs it."""
    from scde_amd import error_models as EM
    groups = np.array([0] * 70 + [1] * 5)
    with pytest.raises(ValueError, match="seed"):
        EM.crossfit_pairs(groups, max_pairs=40, min_pairs_per_cell=3)
    p = EM.crossfit_pairs(groups, max_pairs=40, min_pairs_per_cell=3, seed=1)
    big = p[:, p[0] < 70]
    assert 40 <= big.shape[1] <= 40 + 70 * 3
    assert np.all(big[0] < big[1]) and np.all(big[1] < 70)
    assert len({tuple(x) for x in big.T}) == big.shape[1]
    per_cell = np.bincount(big.ravel(), minlength=70)
    assert per_cell.min() >= 3
    small = p[:, p[0] >= 70]
    assert [tuple(x) for x in small.T] == list(itertools.combinations(range(70, 75), 2))
    np.testing.assert_array_equal(p, EM.crossfit_pairs(groups, max_pairs=40, min_pairs_per_cell=3, seed=1))
    assert not np.array_equal(p, EM.crossfit_pairs(groups, max_pairs=40, min_pairs_per_cell=3, seed=2))
    with pytest.raises(ValueError, match="larger than the population"):
        EM.crossfit_pairs(np.zeros(12, int), max_pairs=20, min_pairs_per_cell=12, seed=1)


def test_pair_lists_round_trip():
    from scde_amd import error_models as EM
    codes = np.array([0, 0, 0, 1, 1, 0], np.int32)
    p = EM._check_pairs(np.array([[2, 0, 3, 5], [0, 1, 4, 2]]), codes)
    off, part = EM._partner_lists(p, 6)
    assert off.tolist() == [0, 2, 3, 5, 6, 7, 8]
    assert [part[off[c]:off[c + 1]].tolist() for c in range(6)] == [[2, 1], [0], [0, 5], [4], [3], [2]]
    back = {(min(c, int(j)), max(c, int(j))) for c in range(6) for j in part[off[c]:off[c + 1]]}
    assert back == {(0, 2), (0, 1), (3, 4), (2, 5)}
    for bad in ([[0], [0]], [[0], [3]], [[0, 1], [1, 0]], [[0], [6]], [[0.5], [1]]):
        with pytest.raises(ValueError):
            EM._check_pairs(np.array(bad), codes)


# ------------------------------------------------------------------ what is not built, and the checks
def test_not_built_and_argument_checks():
    from scde_amd import error_models as EM
    counts = small_counts(60, 6, 0)
    for kw in ({"threshold_segmentation": False}, {"old_cfm": {"a": 1}}, {"save_model_plots": True},
               {"save_crossfit_plots": True}, {"min_count_threshold": 0},
               {"groups": np.array(["a", "a", "a", None, "b", "b"], dtype=object)},
               {"groups": np.array([0, 0, 0, np.nan, 1, 1])}):
        with pytest.raises(NotImplementedError):
            EM.scde_error_models(counts, **kw)
    with pytest.raises(TypeError):
        EM.scde_error_models(counts, no_such_argument=1)
    with pytest.raises(ValueError, match="two cells"):
        EM.scde_error_models(counts, groups=[0, 0, 0, 0, 0, 1], min_size_entries=20)
    with pytest.raises(ValueError, match="one entry per cell"):
        EM.error_model_inputs(counts, groups=[0, 1])
    with pytest.raises(ValueError, match="integer"):
        EM.error_model_inputs(counts, min_count_threshold=1.5)
    with pytest.raises(ValueError, match="min_nonfailed"):
        EM.error_model_inputs(counts, min_nonfailed=-1)
    with pytest.raises(ValueError, match="seed"):
        EM.scde_error_models(counts, max_pairs=3, min_size_entries=20)
    with pytest.raises(ValueError, match="min.size.entries"):
        EM.error_model_inputs(counts)  # 60 genes, 2,000 asked for: R's own stop
    with pytest.raises(ValueError, match="library sizes"):
        EM.error_model_inputs(counts, library_sizes=np.zeros(6))


# ------------------------------------------------------------------ the fit
def test_digamma_trigamma_series():
    """The recurrence and series csrc/device_math.h states, in Python, against scipy."""
    from scipy.special import digamma, polygamma

    def dg(x):
        s = 0.0
        while x < 12:
            s += 1 / x
            x += 1
        r = 1 / x
        r2 = r * r
        p = r2 * (1 / 12 - r2 * (1 / 120 - r2 * (1 / 252 - r2 * (1 / 240 - r2 * (1 / 132 - r2 * (
            691 / 32760 - r2 * (1 / 12)))))))
        return math.log(x) - 0.5 * r - p - s

    def tg(x):
        s = 0.0
        while x < 12:
            s += 1 / (x * x)
            x += 1
        r = 1 / x
        r2 = r * r
        return s + r + 0.5 * r2 + r * r2 * (1 / 6 - r2 * (1 / 30 - r2 * (1 / 42 - r2 * (1 / 30 - r2 * (
            5 / 66 - r2 * (691 / 2730 - r2 * (7 / 6)))))))
    xs = np.r_[np.logspace(-2, 5.2, 300), np.arange(1, 40) * 0.5]
    assert max(abs(dg(x) - digamma(x)) / max(1.0, abs(digamma(x))) for x in xs) <= 2e-15
    assert max(abs(tg(x) - polygamma(1, x)) / polygamma(1, x) for x in xs) <= 2e-15


def test_theta_ml_solves_the_score_equation():
    from scipy.special import digamma
    rng = np.random.default_rng(4)
    mu = np.exp(rng.normal(3, 1, 600))
    y = rng.negative_binomial(2.0, 2.0 / (2.0 + mu)).astype(float)
    w = rng.random(600)
    th = E.theta_ml(y, mu, w)
    score = np.sum(w * (digamma(th + y) - digamma(th) + math.log(th) + 1 - np.log(th + mu) - (y + th) / (mu + th)))
    assert 1.5 < th < 2.7 and abs(score) <= 1e-6 * np.sum(w)


def test_irls_is_the_weighted_maximum_likelihood_fit():
    """At convergence the NB(theta) score in the coefficients vanishes."""
    rng = np.random.default_rng(2)
    l = rng.normal(2, 1.5, 500)
    mu = np.exp(0.4 + 0.8 * l)
    y = rng.negative_binomial(3.0, 3.0 / (3.0 + mu)).astype(float)
    w = rng.random(500)
    coef, st = E.irls(y, l, w, np.log(y + 1 / 6.0 * (y == 0)), 3.0, 200)
    assert st == E.OK and abs(coef[0] - 0.4) < 0.15 and abs(coef[1] - 0.8) < 0.06
    m = np.exp(coef[0] + coef[1] * l)
    g = w * (y - m) / (1 + m / 3.0)
    assert abs(np.sum(g)) <= 1e-5 * np.sum(w) and abs(np.sum(g * l)) <= 1e-5 * np.sum(w)
    assert E.irls(y, np.zeros(500), w, np.log(y + 0.1), None, 20)[1] == E.IRLS_FAILED  # a singular design


def test_restatement_outputs_are_consistent():
    y, x, fp = E.synthetic_cell_nb2(3000, 11)
    f = E.fit_cell_nb2(y, x, fp)
    assert f["status"] == 0 and not f["refit"] and 1 < f["iterations"] < 50
    assert np.all(np.isfinite(f["row"][:6])) and np.all(np.isnan(f["row"][6:])) and f["row"][2] == math.log(0.1)
    assert f["row"][4] > 0 and f["row"][5] >= 0.5 and f["row"][1] > 0  # counts and detection rise with fpm
    assert f["clusters"].shape == y.shape and set(np.unique(f["clusters"])) <= {1, 2}
    np.testing.assert_array_equal(f["clusters"] == 2, 1 - f["p1"] > f["p1"])
    assert np.all((f["p1"] >= 0) & (f["p1"] <= 1)) and np.isfinite(f["llh"])
    one = E.fit_cell_nb2(y, x, fp, iter=1)
    assert one["status"] == 0 and one["iterations"] == 1 and one["llh"] < f["llh"]


def test_the_branches_of_the_fit():
    neg = E.reference_nb2(63, 63, "negative", iter=1)["fit"]
    assert neg["status"] == 0 and neg["negative_slope"] and neg["row"][4] == 0.0
    y, x, fp = E.synthetic_cell_nb2(63, 63, "negative")
    wt = np.where(y <= 1, (1 - fp) / 1e6, 1 - fp)
    assert neg["row"][3] == np.sum(y * wt) / 63 / np.sum(wt)  # a mean, not its log: R's rule
    under = E.reference_nb2(257, 257, "underfit")["fit"]
    assert under["status"] == 0 and under["refit"] and 0 < under["row"][5] < 0.5
    gone = E.reference_nb2(63, 63, "negative")["fit"]  # exp(mean count) as the mean: the likelihood dies
    assert gone["status"] == E.NOT_FINITE and np.all(np.isnan(gone["row"]))
    assert E.fit_cell_nb2(y[:2], x[:2], fp[:2])["status"] == E.TOO_FEW


@pytest.fixture(scope="module")
def esmef_restatement():
    from scde_amd import error_models as EM, knn
    g = golden("esmef_vignette_inputs.npz")
    counts, codes = np.asarray(g["counts"]), np.asarray(g["groups"])
    ls = knn.estimate_library_sizes(counts, 2000, 4)
    inp = E.model_inputs(counts, codes, EM.crossfit_pairs(codes), ls, 4, 3)
    fits = []
    for i in range(counts.shape[1]):
        v = inp["vi"][:, i]
        fits.append(E.fit_cell_nb2(counts[v, i], inp["fpm"][v, i], inp["fail_prior"][v, i]))
    return g["models"], fits


def test_restatement_reproduces_r_on_all_40_cells(esmef_restatement):
    ref, fits = esmef_restatement
    assert all(f["status"] == 0 for f in fits) and not any(f["refit"] for f in fits)
    rows = np.array([f["row"] for f in fits])
    got = distances_to_r(rows, ref)
    for name, fig in got.items():
        print(name, "median %.3g, 90th percentile %.3g, worst %.3g" % fig)
    print("iterations", [f["iterations"] for f in fits])
    np.testing.assert_array_equal(rows[:, 2], ref[:, 2])  # fail.r
    assert np.all(np.isnan(rows[:, 6:])) and np.all(np.isnan(ref[:, 6:]))
    # the recorded table is what was measured (it carries the GPU test's bounds) ...
    for name, fig in got.items():
        for a, b in zip(fig, ESMEF_RESTATEMENT[name]):
            assert a <= b, (name, fig)
    # ... and it says the contract reproduces R: the NB component to six digits in the worst
    # cell, the concomitant to nnet's stopping rule
    assert got["corr.b"][2] < 1e-4 and got["corr.a"][2] < 1e-4 and got["corr.theta"][2] < 1e-4
    assert got["conc.b"][2] < 0.02 and got["conc.a"][2] < 0.01
