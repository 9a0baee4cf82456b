"""pagoda.top.aspects on the host: the Tracy-Widom law of scde_amd/rmt.py, the log-space helpers,
pagoda.effective.cells and the table, against tests/top_aspects_ref.py and mpmath.  No GPU."""
import math

import numpy as np
import pytest

import top_aspects_ref as R
from scde_amd import rmt
from scde_amd import top_aspects as T

TW_POINTS = (-8, -4, -2, 0, 2, 4, 8, 15, 30)


# ------------------------------------------------------------------ Tracy-Widom
def test_airy_constants_and_extended_airy():
    """The two hard-coded constants and the Taylor-stepped Ai against mpmath."""
    import mpmath
    with mpmath.mp.workdps(40):
        assert abs(mpmath.mpf(rmt._AI0) - mpmath.airyai(0)) < 1e-32
        assert abs(mpmath.mpf(rmt._AIP0) - mpmath.airyai(0, derivative=1)) < 1e-32
        us = np.linspace(-16.0, 3.0, 77)
        got = rmt._airy_ld(us)
        for u, g in zip(us, got):
            hi = float(g)
            err = abs(mpmath.airyai(mpmath.mpf(float(u))) - (mpmath.mpf(hi) + mpmath.mpf(float(g - np.longdouble(hi)))))
            # 20 steps of a few np.longdouble roundings each, grown by Bi(3) = 14 at the right end
            assert err < 64 * float(np.finfo(np.longdouble).eps) * 14, (u, float(err))


def test_tw_moments():
    """Mean and variance of the law from its survival function S = exp(ptw_upper_log):
    E X = int_0^inf S - int_-inf^0 (1 - S), E X^2 = 2 int_0^inf x S - 2 int_-inf^0 x (1 - S), by
    48-point Gauss-Legendre rules on [-13, 0] and [0, 16] (beyond them the integrands are below
    1e-30), to 1e-10 of the constants of R/functions.R:2343-2344."""
    x, w = np.polynomial.legendre.leggauss(48)
    m1 = m2 = 0.0
    for lo, hi in ((-13.0, 0.0), (0.0, 16.0)):
        s = lo + 0.5 * (hi - lo) * (x + 1.0)
        ww = 0.5 * (hi - lo) * w
        ls = rmt.ptw_upper_log(s)
        g = np.exp(ls) if lo >= 0 else np.expm1(ls)     # S on the right, -(1 - S) on the left
        m1 += float(np.sum(ww * g))
        m2 += float(np.sum(ww * 2.0 * s * g))
    mean, var = m1, m2 - m1 * m1
    print(f"TW1 mean {mean!r} (error {mean - rmt.TW1_MEAN:.2e}), variance {var!r} (error {var - rmt.TW1_VAR:.2e})")
    assert abs(mean - rmt.TW1_MEAN) < 1e-10
    assert abs(var - rmt.TW1_VAR) < 1e-10


def test_tw_tail_against_mpmath():
    """ptw_upper_log against the 40-digit, 160-node evaluation of the same determinant: 1e-9
    relative.  Measured: 1.5e-11 at s = -8, 3e-12 at s = 30, at most 2e-14 between."""
    worst = 0.0
    for s in TW_POINTS:
        ref = R.tw_upper_log_mp(s)
        got = rmt.ptw_upper_log(float(s))
        err = abs(got - ref) / abs(ref)
        print(f"s = {s}: {got!r} against {ref!r}, relative error {err:.2e}")
        worst = max(worst, err)
    print(f"maximum relative error {worst:.2e}")
    assert worst < 1e-9
    assert abs(rmt.ptw_upper_log(10.0) + 24.79) < 0.01 and abs(rmt.ptw_upper_log(30.0) + 114.06) < 0.01


def test_tw_far_tail():
    """Above s = 40 the trace stands for the determinant: against the 40-digit determinant and
    the product's own determinant path where both hold, across the hand-over, and against the
    leading asymptotic term exp(-(2/3) s^1.5) / (4 sqrt(pi) s^(3/4)) far out."""
    ref = R.tw_upper_log_mp(39)
    far = rmt._tw_upper_log_far(39.0)
    print(f"s = 39: trace {far!r} against {ref!r}, relative error {abs(far - ref) / abs(ref):.2e}")
    assert abs(far - ref) < 1e-9 * abs(ref)
    for s in (25.0, 39.0):
        assert abs(rmt._tw_upper_log_far(s) - rmt.ptw_upper_log(s)) < 1e-10 * abs(rmt.ptw_upper_log(s))
    a, b = rmt.ptw_upper_log(40.0), rmt.ptw_upper_log(40.0 + 1e-7)
    assert 0 < a - b < 1e-7 * 7.0      # the slope is -sqrt(s) - 3 / (4 s) = -6.34
    for s in (120.0, 500.0, 5000.0):   # beyond s = 104 the determinant's matrix is all zeros
        lead = -(2.0 / 3.0) * s ** 1.5 - math.log(4.0 * math.sqrt(math.pi) * s ** 0.75)
        got = rmt.ptw_upper_log(s)
        assert np.isfinite(got) and abs(got - lead) < 1.0 / s ** 1.5, (s, got, lead)   # next term: -(41 / 48) s^-1.5
    assert rmt.ptw_upper_log(1e250) == -np.inf


def test_tw_edges_and_restatement():
    got = rmt.ptw_upper_log(np.array([-np.inf, -20.0, -14.0, np.inf, np.nan]))
    assert got[0] == 0.0 and got[1] == 0.0 and -1e-40 < got[2] <= 0.0 and got[3] == -np.inf and np.isnan(got[4])
    assert isinstance(rmt.ptw_upper_log(0.5), float)
    s = np.array([-3.5, -1.0, 0.7, 3.0, 6.0])
    # the float64 eigenvalue restatement is good to 1e-12 here (tests/top_aspects_ref.py)
    assert np.allclose(rmt.ptw_upper_log(s), R.ptw_upper_log64(s), rtol=1e-11, atol=0)
    assert np.all(np.diff(rmt.ptw_upper_log(np.linspace(-9.0, 40.0, 30))) < 0)


def test_tw_quantile_round_trip():
    for s in (-3.0, -1.27, 0.0, 2.5, 8.0):
        assert abs(rmt.qtw_upper(math.exp(rmt.ptw_upper_log(s))) - s) < 1e-10, s
    assert abs(rmt.qtw_upper(rmt.ptw_upper_log(20.0), log_p=True) - 20.0) < 1e-10
    assert rmt.qtw_upper(1.0) == -np.inf and rmt.qtw_upper(0.0) == np.inf
    with pytest.raises(ValueError):
        rmt.qtw_upper(1.5)
    assert abs(rmt.qtw_upper(0.5) - R.qtw_upper64(0.5)) < 1e-10
    par = rmt.wishart_max_par(40.0, 100)
    assert rmt.q_wishart_max_upper(0.5, 40.0, 100) == par["centering"] + par["scaling"] * rmt.qtw_upper(0.5)


def test_tail_from():
    from scipy.special import gammaincc
    ndf, pdim = 40.0, np.array([100.0, 100.0])
    par = rmt.wishart_max_par(ndf, pdim)
    q = par["centering"] + par["scaling"] * np.array([2.0, 8.0])
    own = rmt.p_wishart_max_upper_log(q, ndf, pdim)
    sw = rmt.p_wishart_max_upper_log(q, ndf, pdim, tail_from=6)
    r8 = math.log(gammaincc(2.0 / 3.0, (2.0 / 3.0) * 8.0 ** 1.5)) + math.lgamma(2.0 / 3.0) + math.log(
        (2.0 / 3.0) ** (1.0 / 3.0))
    assert sw[0] == own[0]
    assert abs(sw[1] - r8) < 1e-9 * abs(r8)        # (q / scaling leaves s = 8 to a few ulp)
    assert abs(own[1] - rmt.ptw_upper_log(8.0)) < 1e-9 * abs(own[1])
    assert 2.0 < sw[1] - own[1] < 3.0              # R's formula lies about 2.5 above the law's tail
    # the continued fraction takes over where gammaincc underflows, without a step
    a = rmt.r_tw_tail_log(np.array([99.0, 102.0, 105.0, 108.0]))   # (2/3) s^1.5 = 657, 687, 717, 748
    assert np.all(np.isfinite(a)) and np.all(np.diff(a) < 0) and np.all(np.abs(np.diff(a, 2)) < 1.0), a


# ------------------------------------------------------------------ log-space helpers
def test_bh_adjust_log():
    rng = np.random.default_rng(3)
    p = rng.uniform(1e-8, 1.0, 60)
    p[[4, 17]] = np.nan
    p[[20, 21]] = 0.03                      # a tie
    got = T.bh_adjust_log(np.log(p))
    want = R.bh_linear(p)
    assert np.isnan(got[4]) and np.isnan(got[17]) and np.isnan(got).sum() == 2
    ok = ~np.isnan(p)
    assert np.allclose(np.exp(got[ok]), want[ok], rtol=1e-13, atol=0)
    assert np.all(got[ok] <= 0)
    assert np.all(np.isnan(T.bh_adjust_log(np.full(3, np.nan))))
    assert T.bh_adjust_log(np.array([-2.0]))[0] == -2.0


def test_qnorm_upper_log():
    from scipy.stats import norm
    z = np.array([-7.0, -1.0, 0.0, 0.5, 3.0, 12.0, 37.0])
    assert np.allclose(T.qnorm_upper_log(norm.logsf(z)), z, rtol=1e-12, atol=1e-12)
    got = T.qnorm_upper_log(-1000.0)
    want = R.qnorm_upper_log_mp(-1000.0)
    assert want > 38.5 and abs(got - want) < 1e-12 * want
    edge = T.qnorm_upper_log(np.array([0.0, -np.inf, np.nan, 0.25]))
    assert edge[0] == -np.inf and edge[1] == np.inf and np.isnan(edge[2]) and np.isnan(edge[3])


def test_pgev_and_gumbel_quantile():
    loc, scale = 0.3, 0.7
    t = np.array([1.0, 0.0, -1e-3, -2.0, -4.999, -5.0, -5.001, -40.0])   # gev.t before the clamp
    x = loc - scale * t
    got = T.pgev_upper_log(x, loc, scale)
    tt = np.minimum(0.0, -(x - loc) / scale)
    want = np.where((tt > -5) & (tt < 0), np.log(-np.expm1(-np.exp(tt))), tt)
    assert np.array_equal(got, want)
    assert got[0] == 0.0 and got[1] == 0.0 and got[-1] == tt[-1]
    assert got[4] != tt[4] and got[6] == tt[6]                           # the two sides of the switch
    assert abs(got[4] - got[6]) < 0.01
    assert np.array_equal(got, R.pgev_upper_log(x, loc, scale))
    # a shape that is not 0
    g = T.pgev_upper_log(np.array([2.0]), 0.0, 1.0, shape=0.1)[0]
    tv = -math.log(1.2) / 0.1
    assert abs(g - math.log(-math.expm1(-math.exp(tv)))) < 1e-15
    # the Gumbel upper quantile inverts the upper tail
    for p in (0.4, 0.025, 1e-9):
        q = T.qgumbel_upper(p, loc, scale)
        assert abs(-math.expm1(-math.exp(-(q - loc) / scale)) - p) < 1e-12 * p


def test_qchisq_upper_log_deep_tail():
    import mpmath
    from scipy.stats import chi2
    df = 40.5
    lp = np.array([-1.0, -50.0, -599.0, -601.0, -2000.0])
    x = T.qchisq_upper_log(lp, df)
    assert np.allclose(chi2.logsf(x[:3], df), lp[:3], rtol=1e-11, atol=0)
    with mpmath.mp.workdps(30):
        for l, v in zip(lp[3:], x[3:]):
            ref = mpmath.log(mpmath.gammainc(df / 2, v / 2, mpmath.inf, regularized=True))
            assert abs(float(ref) - l) < 1e-11 * abs(l)
    assert 0 < x[3] - x[2] < 6   # no step at the hand-over (d x / d lp is about -2.1 here)
    assert T.qchisq_upper_log(-np.inf, df) == np.inf and T.qchisq_upper_log(0.0, df) == 0.0


# ------------------------------------------------------------------ pagoda.effective.cells
def _eff_pwpca(sn0, factor=1.0, cells=60):
    pw = {}
    for j, n in enumerate((10, 20, 50, 100, 200, 400)):
        v = R.effective_cells_fit(sn0, np.full(5, math.sqrt(n - 0.5))) * factor
        pw[f"s{j}"] = {"z": np.sqrt(v)[:, None], "n": n, "xp": {"scores": np.zeros((cells, 1))}}
    pw["empty"] = None
    return pw


def test_effective_cells():
    sn0 = 6.3
    pw = _eff_pwpca(sn0)
    want = sn0 ** 2 + 0.5
    assert abs(T.pagoda_effective_cells(pw) - want) < 1e-8 * want                # from the upper bound
    assert abs(T.pagoda_effective_cells(pw, start=3.0) - want) < 1e-8 * want     # from below
    assert abs(T.pagoda_effective_cells(pw, start=20.0) - want) < 1e-8 * want
    # the restated objective is the one minimised
    v = np.concatenate([x["z"][:, 0] ** 2 for x in pw.values() if x is not None])
    sp = np.concatenate([np.full(5, math.sqrt(x["n"] - 0.5)) for x in pw.values() if x is not None])
    for sn in (1.0, 4.0, 33.0):
        assert abs(T._effective_cells_terms(sn, v, sp)[0] - R.effective_cells_objective(sn, v, sp)) <= 1e-12 * (
            R.effective_cells_objective(sn, v, sp))
        h = 1e-6 * sn
        num = (R.effective_cells_objective(sn + h, v, sp) - R.effective_cells_objective(sn - h, v, sp)) / (2 * h)
        assert abs(T._effective_cells_terms(sn, v, sp)[1] - num) < 1e-5 * abs(num)
    # variances far above the model at every sn: the descent ends at the lower bound, sn = 1
    assert T.pagoda_effective_cells(_eff_pwpca(sn0, factor=900.0)) == 1.5
    # variances below the model at sn = cells: nothing lower to the left of the upper bound
    assert T.pagoda_effective_cells(_eff_pwpca(sn0, factor=1e-3)) == 60.0 ** 2 + 0.5
    with pytest.raises(ValueError):
        T.pagoda_effective_cells({"a": None})


# ------------------------------------------------------------------ the table
CELLS = 40
SIZES = (10, 14, 20, 33, 50, 75, 100, 150, 220, 300, 400)   # 11 sets and one None entry


def make_pwpca(seed=5):
    rng = np.random.default_rng(seed)
    center = rmt.q_wishart_max_upper(0.5, float(CELLS), np.array(SIZES, dtype=np.float64))
    pw = {}
    for j, n in enumerate(SIZES):
        # (the scaled statistic stays above -4, where the float64 restatement of the law holds)
        f = np.array([rng.uniform(0.95, 1.25), rng.uniform(0.95, 1.05)])
        if j == 2:
            f[0] = 3.0          # two sets several times above the expectation
        if j == 4:
            f[0] = 2.5
        var = center[j] * f
        rot = rng.normal(size=(n, 2))
        xp = {"scores": rng.normal(size=(CELLS, 2)), "scoreweights": rng.uniform(0.2, 1.0, size=(CELLS, 2)),
              "rotation": rot, "rotation_names": [f"g{(7 * j + k) % 450}" for k in range(n)]}
        if j % 3 == 0:
            xp["randvar"] = var[0] * rng.uniform(0.2, 0.6, size=6)
        pw[f"set{j}"] = {"xp": xp, "sd": np.sqrt(var)[None, :], "n": n, "z": np.sqrt(rng.uniform(1, 3, size=(10, 1)))}
        if j == 5:
            pw["nothing"] = None
    # the max / 3 rule with a tie at the threshold (exact in binary)
    r = pw["set2"]["xp"]["rotation"]
    r[:, 0] = 0.1
    r[0, 0], r[1, 0], r[2, 0], r[3, 0] = -0.75, 0.25, -0.25, 0.2499
    return pw


def make_clpca(seed=9):
    rng = np.random.default_rng(seed)
    n = rng.integers(5, 80, size=30)
    par = rmt.wishart_max_par(float(CELLS), n)
    var = par["centering"] + par["scaling"] * (rmt.TW1_MEAN + rng.gumbel(0.0, 1.0, size=30))
    varm, clvlm, _ = rmt.score_varm({"n": n, "var": var, "round": np.repeat(np.arange(6), 5)}, float(CELLS))
    goc = {}
    for k, size in enumerate((8, 15, 25, 40, 60)):
        p = rmt.wishart_max_par(float(CELLS), size)
        v = float(p["centering"]) * (2.2 if k == 1 else rng.uniform(0.8, 1.1))
        xp = {"scores": rng.normal(size=(CELLS, 1)), "scoreweights": rng.uniform(0.2, 1.0, size=(CELLS, 1)),
              "rotation": rng.normal(size=(size, 1)), "rotation_names": [f"g{(11 * k + i) % 450}" for i in range(size)]}
        if k == 0:
            xp["randvar"] = v * rng.uniform(0.2, 0.6, size=5)
        goc[f"geneCluster.{k + 1}"] = {"xp": xp, "sd": np.array([[math.sqrt(v)]]), "n": size}
    return {"cl.goc": goc, "varm": varm, "clvlm": clvlm}


# What the columns may differ by.  The restatement's Tracy-Widom log tail is good to 1e-12 and the
# product's is held to 1e-9 (test_tw_tail_against_mpmath); d z = d lp / (phi / S)(z), the hazard
# being above 0.5 for z >= -1 and above z for large z while |lp| <= 1 + z^2, so a relative 1e-9 in
# lp is below 4e-9 (1 + |z|) in z.  The quantiles are roots to 1e-12.
TOL = {"shz": 1e-13, "exp": 1e-10, "ub": 1e-10, "ub_stringent": 1e-10, "score": 1e-10, "oec": 1e-10}


def _check_columns(t, ref):
    for k in ("i", "var", "n", "npc"):
        assert np.array_equal(np.asarray(t[k], dtype=np.float64), ref[k]), k
    for k, tol in TOL.items():
        assert np.allclose(t[k], ref[k], rtol=tol, atol=0, equal_nan=True), k
    for k in ("z", "cz", "adj_shz"):
        ok = np.isfinite(ref[k])
        assert np.array_equal(np.isnan(t[k]), np.isnan(ref[k])), k
        assert np.array_equal(t[k][np.isinf(ref[k])], ref[k][np.isinf(ref[k])]), k
        assert np.all(np.abs(t[k][ok] - ref[k][ok]) <= 4e-9 * (1.0 + np.abs(ref[k][ok]))), k


@pytest.fixture(scope="module")
def pw():
    return make_pwpca()


@pytest.fixture(scope="module")
def pw_ref(pw):
    return R.table(pw, float(CELLS))


def test_table_pathway_side(pw, pw_ref):
    t = T.top_aspects_table(pw, n_cells=CELLS)
    assert len(t["var"]) == 22 and t["n_cells"] == CELLS
    _check_columns(t, pw_ref)
    assert t["name"][:4] == ["set0", "set0", "set1", "set1"] and t["name"][12] == "set6"   # the None entry is skipped
    assert np.isnan(t["shz"]).sum() == 14 and np.isnan(t["adj_shz"]).sum() == 14
    assert np.all(t["ub_stringent"] > t["ub"]) and np.all(t["ub"] > t["exp"])
    # the two planted sets stand out; nothing is within reach of the threshold, so valid is exact
    for adjust in (True, False):
        tt = T.top_aspects_table(pw, n_cells=CELLS, adjust_scores=adjust)
        col = pw_ref["cz" if adjust else "z"]
        assert np.all(np.abs(col - T.Z_SCORE) > 1e-3)
        assert np.array_equal(tt["valid"], col >= T.Z_SCORE)
        assert tt["valid"][4] and tt["valid"][8]
    assert T.top_aspects_table(pw, n_cells=CELLS, adjust_scores=False)["valid"].sum() >= t["valid"].sum()
    # tail_from reaches the table
    tf = T.top_aspects_table(pw, n_cells=CELLS, tw_tail_from=6.0)
    _check_columns(tf, R.table(pw, float(CELLS), tail_from=6.0))
    assert tf["z"][4] < t["z"][4] and tf["z"][0] == t["z"][0]


def test_table_without_n_cells_uses_effective_cells(pw):
    t = T.top_aspects_table(pw, z_score=-50.0)
    assert t["n_cells"] == T.pagoda_effective_cells(pw)
    t2 = T.top_aspects_table(pw, z_score=-50.0, effective_cells_start=5.0)
    assert t2["n_cells"] == T.pagoda_effective_cells(pw, start=5.0)


def test_return_table_names_and_genes(pw, pw_ref):
    valid = np.nonzero(pw_ref["cz"] >= T.Z_SCORE)[0]
    df = T.pagoda_top_aspects(pw, n_cells=CELLS, return_table=True)
    assert list(df.columns) == ["name", "npc", "n", "score", "z", "adj.z", "sh.z", "adj.sh.z"]
    order = valid[np.argsort(-pw_ref["score"][valid], kind="stable")]
    assert list(df["npc"]) == [int(v) for v in pw_ref["npc"][order]]
    assert list(df["n"]) == [int(v) for v in pw_ref["n"][order]]
    assert np.allclose(df["score"], pw_ref["score"][order], rtol=1e-10)
    assert np.all(np.diff(df["score"].to_numpy()) <= 0)
    assert set(df["name"]) >= {"set2", "set4"}
    # a low threshold keeps every row: ties in score would keep table order (stable sort)
    full = T.pagoda_top_aspects(pw, n_cells=CELLS, return_table=True, z_score=-50.0)
    assert len(full) == 22
    # gw: per valid row the |loadings| >= max / 3 (the tie at exactly max / 3 is kept), per gene the maximum
    gw = T.pagoda_top_aspects(pw, n_cells=CELLS, return_genes=True)
    assert list(gw) == sorted(gw)
    names2 = pw["set2"]["xp"]["rotation_names"]
    for k, want in ((0, 0.75), (1, 0.25), (2, 0.25)):
        assert gw[names2[k]] >= want
    want = {}
    sets = [x for x in pw.values() if x is not None]
    for r in valid:
        x = sets[int(pw_ref["i"][r]) - 1]
        s = np.abs(x["xp"]["rotation"][:, int(pw_ref["npc"][r]) - 1])
        for g, v in zip(x["xp"]["rotation_names"], s):
            if v >= s.max() / 3:
                want[g] = max(want.get(g, 0.0), float(v))
    assert gw == want
    only2 = T.pagoda_top_aspects({"set2": pw["set2"], "set0": pw["set0"], "set1": pw["set1"]}, n_cells=CELLS,
                                 return_genes=True)
    assert names2[3] not in only2 and only2[names2[1]] == 0.25 and only2[names2[2]] == 0.25   # 0.2499 falls out
    with pytest.raises(ValueError, match="no significantly overdispersed pathways found at z.score threshold of"):
        T.pagoda_top_aspects(pw, n_cells=CELLS, z_score=1e3, return_table=True)


def test_table_cluster_side(pw):
    cl = make_clpca()
    xf = rmt.gumbel_fit(cl["varm"]["varst"])
    ref = R.table(pw, float(CELLS), clpca=cl, gumbel=(xf["location"], xf["scale"]))
    t = T.top_aspects_table(pw, cl, n_cells=CELLS)
    assert len(t["var"]) == 27
    _check_columns(t, ref)
    assert list(t["i"][22:]) == [12, 13, 14, 15, 16]            # shifted past the 11 gene sets
    assert t["name"][22:] == [f"geneCluster.{k}" for k in range(1, 6)]
    # the pathway rows' cz is adjusted among themselves: as without the clusters
    alone = T.top_aspects_table(pw, n_cells=CELLS)
    assert np.array_equal(t["cz"][:22], alone["cz"]) and np.array_equal(t["ub_stringent"][:22], alone["ub_stringent"])
    # adj_shz runs over all rows
    assert np.isnan(t["adj_shz"]).sum() == 14 + 4
    assert t["valid"][23] and np.all(t["ub_stringent"][22:] > t["ub"][22:])
    df = T.pagoda_top_aspects(pw, cl, n_cells=CELLS, return_table=True)
    assert "geneCluster.2" in set(df["name"])
