"""CPU tests of pagoda.varnorm's host parts: the edf table and its fixture, the .rda reader's
byte-code extension, the trend smoother and the chi-squared maps (scde_amd/varnorm.py)."""
import os
import sys

import numpy as np
import pytest
from scipy.stats import chi2

from conftest import GOLD, ROOT, golden

import varnorm_ref as R
from scde_amd import varnorm as V

REFERENCE = os.environ.get("SCDE_REFERENCE", "/root/reference")
EDFF_RDA = os.path.join(REFERENCE, "data", "scde.edff.rda")


# ------------------------------------------------------------------ the fixture
def test_edf_fixture_is_the_uniform_grid_of_the_gam():
    g = golden("scde_edff.npz")
    lt, y = g["lt"], g["log_edf"]
    assert lt.shape == y.shape == (1000,)
    d = np.diff(lt)
    assert np.all(d > 0)
    assert np.max(np.abs(d - d.mean())) < 1e-12
    assert abs(d.mean() - 0.0115244) < 1e-7
    assert abs(lt[0] - np.log(1e-2)) < 1e-12 and abs(lt[-1] - np.log(1e3)) < 1e-12
    e = np.exp(y)
    assert 0.0036 < e.min() < 0.0037 and 1.008 < e.max() < 1.01


def test_spline_interpolates_the_table_and_is_natural():
    g = golden("scde_edff.npz")
    ref = R.EdfSpline(g["lt"], g["log_edf"])
    np.testing.assert_allclose(ref.log_edf(g["lt"]), g["log_edf"], rtol=0, atol=1e-14)
    assert abs(float(ref.cs(g["lt"][0], 2))) < 1e-9 and abs(float(ref.cs(g["lt"][-1], 2))) < 1e-9
    # the library's table: the same curve between the knots, and linear beyond the ends
    tab = V.load_edf_table(os.path.join(GOLD, "scde_edff.npz"))
    assert tab.m2[0] == 0.0 and tab.m2[-1] == 0.0
    x = np.concatenate([np.linspace(g["lt"][0] - 3, g["lt"][-1] + 3, 4001), g["lt"], g["lt"][:-1] + 1e-9])
    # the end slope is a difference of neighbouring table values (|y| <= 5.7) over h = 0.0115: it carries
    # about eps * 5.7 / h = 1e-13 relative, times the 3 units extrapolated, times a few roundings
    np.testing.assert_allclose(tab.log_edf_at(x), ref.log_edf(x), rtol=0, atol=3e-12)
    inside = (x >= g["lt"][0]) & (x <= g["lt"][-1])
    np.testing.assert_allclose(tab.log_edf_at(x[inside]), ref.log_edf(x[inside]), rtol=0, atol=2e-14)
    out = np.array([g["lt"][0] - 1.0, g["lt"][0] - 2.0, g["lt"][0] - 3.0])
    s = tab.log_edf_at(out)
    assert abs((s[0] - s[1]) - (s[1] - s[2])) < 1e-13
    th = np.array([1e-3, 1e-2, 0.5, 1.0, 999.0, 1000.0, 1000.0001, 1e4, np.inf])
    np.testing.assert_allclose(tab(th), ref.edf(th), rtol=1e-12)
    assert np.all(tab(th)[-3:] == 1.0)


def test_edf_table_rejects_a_grid_that_is_not_uniform():
    g = golden("scde_edff.npz")
    lt = g["lt"].copy()
    lt[500] += 1e-4
    with pytest.raises(ValueError):
        V.EdfTable(lt, g["log_edf"])
    with pytest.raises(TypeError):
        V._check_edff({"lt": lt})


@pytest.mark.skipif(not os.path.exists(EDFF_RDA), reason="the reference tree is absent")
def test_rdata_reads_the_gam_and_the_tool_reproduces_the_fixture(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_edff_table
    import rdata
    gam = rdata.read_rda(EDFF_RDA)["scde.edff"]          # byte-compiled closures inside: SEXP type 21
    names = gam.attrs["names"].value
    assert {"fitted.values", "model", "smooth", "family"} <= set(names)
    assert "gam" in gam.attrs["class"].value
    out = tmp_path / "edff.npz"
    make_edff_table.main([EDFF_RDA, str(out)])
    got, want = np.load(out), golden("scde_edff.npz")
    assert np.array_equal(got["lt"], want["lt"]) and np.array_equal(got["log_edf"], want["log_edf"])


# ------------------------------------------------------------------ fit_trend
def _curve(x):
    return 0.8 - 0.6 * x + 0.3 * np.sin(1.5 * x)


def test_fit_trend_recovers_a_smooth_curve():
    rng = np.random.default_rng(5)
    n = 1500
    x = np.sort(rng.uniform(-2, 4, n))
    w = rng.uniform(0.2, 3.0, n)
    y = _curve(x) + rng.normal(0, 0.15, n) / np.sqrt(w)
    tr = V.fit_trend(x, y, weights=w, k=10)
    xs = np.linspace(-1.9, 3.9, 200)
    assert np.max(np.abs(tr.predict(xs) - _curve(xs))) < 0.05      # noise sd / sqrt(n / k) ~ 0.012
    assert 3 < tr.edf <= 10
    # beyond the end knots the curve is a straight line
    out = tr.predict(np.array([5.0, 6.0, 7.0]))
    assert abs((out[2] - out[1]) - (out[1] - out[0])) < 1e-10


def test_fit_trend_ignores_points_of_weight_zero():
    rng = np.random.default_rng(6)
    x = rng.uniform(0, 3, 300)
    y = _curve(x) + rng.normal(0, 0.1, 300)
    w = rng.uniform(0.5, 2, 300)
    base = V.fit_trend(x, y, weights=w)
    x2, y2, w2 = np.append(x, [1.5, 9.0]), np.append(y, [50.0, -80.0]), np.append(w, [0.0, 0.0])
    with_zero = V.fit_trend(x2, y2, weights=w2)
    xs = np.linspace(0, 3, 50)
    assert np.array_equal(base.predict(xs), with_zero.predict(xs))
    assert base.lam == with_zero.lam


def test_fit_trend_penalises_pure_noise_harder():
    rng = np.random.default_rng(7)
    x = np.sort(rng.uniform(-2, 4, 800))
    clean = V.fit_trend(x, _curve(x) + rng.normal(0, 0.01, 800))
    noise = V.fit_trend(x, rng.normal(0, 1.0, 800))
    assert noise.lam > 10 * clean.lam
    assert noise.edf < clean.edf


def test_trend_argument_bypasses_the_smoother(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("fit_trend called although trend= was given")
    monkeypatch.setattr(V, "fit_trend", boom)
    rng = np.random.default_rng(8)
    N, C = 50, 30
    av = rng.uniform(0.5, 200, N)
    mom = {"edf": rng.uniform(2, C, N), "wvar": rng.uniform(0.5, 5, N) * av, "rowsum_matw": rng.uniform(1, C, N)}
    trend = np.log10(mom["wvar"] / av ** 2) - rng.normal(0, 0.2, N)
    st = V.varnorm_statistics(av, mom, C, trend=trend)
    ref = R.statistics(av, mom, C, trend)
    assert np.array_equal(st["vi"], ref["vi"]) and st["vi"].all()
    np.testing.assert_allclose(st["zval"], ref["zval"], rtol=1e-14)
    np.testing.assert_allclose(st["arv"], ref["arv"], rtol=1e-10)
    with pytest.raises(ValueError):
        V.varnorm_statistics(av, mom, C, trend=trend[:-1])
    with pytest.raises(AssertionError):
        V.varnorm_statistics(av, mom, C)


def test_statistics_fit_genes_and_the_empty_fit():
    rng = np.random.default_rng(9)
    N, C = 200, 40
    av = rng.uniform(0.5, 200, N)
    mom = {"edf": rng.uniform(2, C, N), "wvar": rng.uniform(0.5, 5, N) * av, "rowsum_matw": rng.uniform(1, C, N)}
    mom["wvar"][3] = 0.0          # not valid: wvar must be positive
    mom["wvar"][4] = np.nan
    mom["rowsum_matw"][5] = 0.0
    st = V.varnorm_statistics(av, mom, C)
    assert not st["vi"][3] and not st["vi"][4] and not st["vi"][5] and st["vi"].sum() == N - 3
    assert np.isnan(st["arv"][[3, 4, 5]]).all() and np.isfinite(st["arv"][st["vi"]]).all()
    mask = np.zeros(N, bool)
    mask[:60] = True
    sub = V.varnorm_statistics(av, mom, C, fit_mask=mask)
    assert np.array_equal(sub["vi"], st["vi"]) and not np.array_equal(sub["trend"], st["trend"])
    und = V.varnorm_statistics(av, mom, C, minimize_underdispersion=True)
    assert np.isfinite(und["arv"][und["vi"]]).all()
    from scde_amd import ScdeError
    with pytest.raises(ScdeError):
        V.varnorm_statistics(av, mom, C, fit_mask=np.zeros(N, bool))
    with pytest.raises(NotImplementedError):
        V.pagoda_varnorm({}, np.zeros((2, 2), np.int32), None, gene_length=np.ones(2))


def test_holm_is_p_adjust():
    p = np.array([0.01, 0.04, 0.03, 0.5, 0.002])
    # p.adjust(c(0.01, 0.04, 0.03, 0.5, 0.002)): sorted p times (n - rank + 1), running maximum, capped at 1
    np.testing.assert_allclose(V._holm(p), [0.04, 0.09, 0.09, 0.5, 0.01], rtol=1e-15)


# ------------------------------------------------------------------ the chi-squared maps
def test_adjusted_variance_equals_isf_of_sf_where_representable():
    C = 40
    z, e = np.meshgrid(np.geomspace(0.2, 5, 25), np.array([1.5, 3.0, 10.0, 25.0, 39.0]))
    z, e = z.ravel(), e.ravel()
    sf = chi2.sf(z * (e - 1), e)
    ok = (sf > 1e-250) & (sf < 1 - 1e-9)
    want = np.minimum(10.0, chi2.isf(sf[ok], C - 1) / C)
    got = V.adjusted_variance(z[ok], e[ok], C, 10.0)
    # isf(sf()) loses digits where sf is close to 1 (1 - sf carries the information): its own error there
    # is ulp(1) / (1 - sf) relative in the probability; compare where that is below 1e-10
    fine = (1 - sf[ok]) > 1e-4
    np.testing.assert_allclose(got[fine], want[fine], rtol=1e-9)
    np.testing.assert_allclose(got, R.adjusted_variance(z[ok], e[ok], C, 10.0), rtol=1e-10)


def test_adjusted_variance_edges():
    C = 40
    assert V.adjusted_variance(np.array([1e9]), np.array([20.0]), C, 10.0)[0] == 10.0
    assert V.adjusted_variance(np.array([1e9]), np.array([20.0]), C, 5.0)[0] == 5.0
    assert np.all(V.adjusted_variance(np.array([0.5, 3.0, 1e6]), np.array([1.0, 0.5, 1.0]), C, 10.0) == 0.0)
    assert V.adjusted_variance(np.array([1e-12]), np.array([30.0]), C, 10.0)[0] == 0.0   # |qv| < 1e-10


@pytest.mark.parametrize("C", [37, 130, 2000])
def test_adjusted_variance_is_finite_over_the_grid(C):
    z, e = np.meshgrid(np.geomspace(1e-6, 1e6, 49), np.geomspace(0.5, 2000, 40))
    got = V.adjusted_variance(z.ravel(), e.ravel(), C, 10.0)
    assert np.all(np.isfinite(got)) and got.min() >= 0.0 and got.max() <= 10.0
    # increasing in zval at a fixed edf
    g = got.reshape(z.shape)
    assert np.all(np.diff(g, axis=1) >= -1e-12)
