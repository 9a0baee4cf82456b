"""GPU tests of pagoda.varnorm after its weights stage (k_varnorm_moments, k_varnorm_matrix, the
host statistics between them) and of pagoda.subtract.aspect, against tests/varnorm_ref.py.

The reference takes the stage-1 outputs of the same inputs (``pagoda_varnorm_weights``, whose
results repeat bit for bit), so only the new stages are compared.  Shapes: 70 and 130 genes (one
and three 64-gene blocks, the last ragged), 37 and 130 cells (neither a multiple of the 8 waves
that share a gene block).  Every case holds a gene without counts and a gene whose counts are
round(mu) in every cell.  The comparisons pass ``trend=`` so that no GCV minimum can flip on a
last-bit difference; one test runs the built-in smoother.

Bounds (from the issue that added these stages): edf, wvar, bwvar_ratio rtol 1e-10 (a dozen FP64
operations per element, device exp / log / pow a few ulp from libm, sums of at most 130 terms of
one sign); arv, mat, matw rtol 1e-8 (the pchisq -> qchisq map amplifies wvar's error by at most
the order of edf <= C), atol 1e-12 on mat; NaN positions and vi exact.
"""
import os

import numpy as np
import pytest

from conftest import GOLD, golden

import varnorm_ref as R

pytestmark = pytest.mark.gpu

NRAND = 20


def _models(kind):
    from oracle import oracle as O
    g = golden("knn300.npz" if kind == "local" else "esmef500.npz")
    cols = {c: g["models"][:, j].copy() for j, c in enumerate(O.MODEL_COLUMNS) if not np.all(np.isnan(g["models"][:, j]))}
    return g, cols


def make_inputs(kind, N, C, big_theta=False):
    """Models (12-column local-theta ones from knn300, constant-theta ones from esmef500) tiled to
    C cells with a small deterministic change per repeat, and counts of N expressed genes."""
    g, cols = _models(kind)
    nc = g["models"].shape[0]
    idx = np.arange(C) % nc
    rep = (np.arange(C) // nc).astype(np.float64)
    models = {k: v[idx].copy() for k, v in cols.items()}
    models["corr.b"] = models["corr.b"] + 0.05 * rep
    models["fail.r"] = models["fail.r"] - 0.1 * rep
    if big_theta:   # theta above 1e3 in some cells: the edf = 1 branch (with theta_range[1] = 1e4)
        models["corr.theta"][::3] = 5e3
        models["corr.theta"][1::7] = 2e4
    counts = np.asarray(g["counts"])
    expressed = np.argsort(-(counts > 0).sum(1), kind="stable")[:N]
    cd = np.ascontiguousarray(counts[np.sort(expressed)][:, idx]).astype(np.int32)
    rng = np.random.default_rng(100 + N + C)
    cd = (cd * rng.uniform(0.7, 1.3, cd.shape)).astype(np.int32)   # the repeated cells differ
    cd[3] = 0                                                        # a gene without counts
    with np.errstate(over="ignore"):
        cd[7] = np.rint(np.exp(3.0 * models["corr.a"] + models["corr.b"])).astype(np.int32)   # counts = round(mu)
    prior = {"x": g["prior_x"], "y": g["prior_y"]}
    return models, cd, prior


def edf_tables():
    from scde_amd import varnorm as V
    g = golden("scde_edff.npz")
    return V.load_edf_table(os.path.join(GOLD, "scde_edff.npz")), R.EdfSpline(g["lt"], g["log_edf"])


def stage1(models, cd, prior, batch):
    from scde_amd import api
    from scde_amd import pagoda as PG
    api.set_rand("glibc")
    return PG.pagoda_varnorm_weights(models, cd, prior, batch=batch, n_cores=1, n_randomizations=NRAND)


def quadratic_trend(models, cd, s1, codes=None, **kw):
    """An explicit ``trend=``: the least-squares parabola of the restatement's cv2 on the log10
    modes.  Both sides are given the same vector, so no smoother takes part in a comparison."""
    _, ref_edf = edf_tables()
    mom = R.moments(models, cd, ref_edf, s1["avmodes"], s1["matw"], s1.get("modes"), s1.get("bmatw"), codes, **kw)
    wvar = mom["bwvar"] if codes is not None else mom["wvar"]
    with np.errstate(all="ignore"):
        lev, cv2 = np.log10(s1["avmodes"]), np.log10(wvar / s1["avmodes"] ** 2)
    ok = np.isfinite(lev) & np.isfinite(cv2)
    return np.where(np.isfinite(lev), np.polyval(np.polyfit(lev[ok], cv2[ok], 2), lev), 0.0)


def _batch(kind, C):
    if kind is None:
        return None, None
    if kind == "three":   # the single cell of level "z" joins the largest level, "a"
        b = np.array(["a" if i % 5 < 3 else "b" for i in range(C)], dtype=object)
        b[4] = "z"
        merged = np.where(b == "z", "a", b)
    else:
        b = np.array(["p" if i % 2 else "q" for i in range(C)], dtype=object)
        merged = b
    levels = sorted(set(merged.tolist()))
    return b, np.array([levels.index(v) for v in merged], np.int32)


CASES = {
    "local_70x37": dict(kind="local", N=70, C=37),
    "local_130x130_three_levels": dict(kind="local", N=130, C=130, batch="three"),
    "const_130x37_two_levels_power": dict(kind="const", N=130, C=37, batch="two", weight_df_power=0.5),
    "const_70x130_theta_1e4": dict(kind="const", N=70, C=130, big_theta=True, theta_range=(1e-2, 1e4)),
    "local_130x37_fit_genes": dict(kind="local", N=130, C=37, fit=True, weight_k=0.7, max_adj_var=5),
    "const_70x37_trim": dict(kind="const", N=70, C=37, trim=True),
}


def run_case(case):
    """(library result, reference result) of one case."""
    from scde_amd import varnorm as V
    c = dict(CASES[case])
    models, cd, prior = make_inputs(c["kind"], c["N"], c["C"], c.get("big_theta", False))
    C = c["C"]
    batch, codes = _batch(c.get("batch"), C)
    tab, ref_edf = edf_tables()
    trim = 0
    cd_ref = cd
    if c.get("trim"):
        trim = 3.0 / C
        cd = cd.copy()
        cd[11] = 0
        cd[11, [2, 9, 30]] = (40, 7, 300)        # three cells only: Winsorized away, the gene drops out
        cd_ref, kept_ref = R.trim_counts(models, cd, trim)
        assert 11 not in kept_ref and 3 not in kept_ref and len(kept_ref) == c["N"] - 2
    s1 = stage1(models, cd_ref, prior, batch)
    trend = quadratic_trend(models, cd_ref, s1, codes, weight_df_power=c.get("weight_df_power", 1),
                            theta_range=c.get("theta_range", (1e-2, 1e2)))
    fit_mask = None
    fit_genes = None
    if c.get("fit"):
        fit_genes = list(range(5, c["N"], 3))
        fit_mask = np.zeros(c["N"], bool)
        fit_mask[fit_genes] = True
    kw = dict(weight_k=c.get("weight_k", 0.9), weight_df_power=c.get("weight_df_power", 1),
              max_adj_var=c.get("max_adj_var", 10), theta_range=c.get("theta_range", (1e-2, 1e2)))
    got = V.pagoda_varnorm(models, cd, tab, batch=batch, trim=trim, prior=prior, fit_genes=fit_genes, n_cores=1,
                           n_randomizations=NRAND, trend=trend, return_details=True, **kw)
    want = R.varnorm(models, cd_ref, ref_edf, s1, codes, trend, fit_mask, **kw)
    if c.get("trim"):
        assert np.array_equal(got["kept"], kept_ref)
    return got, want, s1, trend


_results = {}


def case_results(case):
    if case not in _results:
        _results[case] = run_case(case)
    return _results[case]


def _report(name, got, want):
    with np.errstate(all="ignore"):
        rel = np.abs(got - want) / np.abs(want)
    rel = rel[np.isfinite(rel)]
    print(f"  {name}: max relative error {rel.max() if rel.size else 0.0:.3g}")


@pytest.mark.parametrize("case", list(CASES))
def test_varnorm_matches_the_restatement(case):
    got, want, s1, _ = case_results(case)
    mom = want["mom"]
    batched = "bwvar" in mom
    print(case)
    # stage 1 as the library ran it inside is stage 1 as the reference was given it
    assert np.array_equal(got["avmodes"], s1["avmodes"])
    _report("edf", got["edf"], mom["edf"])
    _report("wvar", got["wvar"], want["wvar"])
    _report("arv", got["arv"], want["arv"])
    _report("mat", got["mat"], want["mat"])
    _report("matw", got["matw"], want["matw"])
    np.testing.assert_allclose(got["edf"], mom["edf"], rtol=1e-10)
    np.testing.assert_allclose(got["wvar"], want["wvar"], rtol=1e-10)
    if batched:
        _report("bwvar_ratio", got["bwvar_ratio"], mom["bwvar_ratio"])
        np.testing.assert_allclose(got["bwvar_ratio"], mom["bwvar_ratio"], rtol=1e-10)
        assert got["modes"].shape == (int(np.max(_batch(CASES[case]["batch"], CASES[case]["C"])[1])) + 1,
                                      got["mat"].shape[0])
    else:
        assert "bwvar_ratio" not in got
    assert np.array_equal(got["vi"], want["vi"])
    assert got["vi"].sum() >= got["vi"].size // 2
    assert np.array_equal(np.isnan(got["arv"]), np.isnan(want["arv"]))
    assert np.array_equal(np.isnan(got["mat"]), np.isnan(want["mat"]))
    assert not np.isnan(got["matw"]).any() and not np.isinf(got["arv"]).any()
    np.testing.assert_allclose(got["zval"], want["zval"], rtol=1e-9)
    np.testing.assert_allclose(got["arv"], want["arv"], rtol=1e-8)
    np.testing.assert_allclose(got["mat"], want["mat"], rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(got["matw"], want["matw"], rtol=1e-8)
    # what the cases are there for
    v = got["vi"]
    assert np.isfinite(got["mat"][v]).all()
    assert np.sum(got["arv"][v] > 0) > v.sum() // 4 and np.sum(np.abs(got["mat"][v]).max(1) > 0) > v.sum() // 4
    if CASES[case].get("max_adj_var"):
        assert np.nanmax(got["arv"]) <= 5.0
    if not CASES[case].get("trim"):
        assert np.all(got["mat"][3][np.isfinite(got["mat"][3])] == 0.0)   # no counts: x = 0 in every cell


def test_edf_one_branch_is_taken():
    """theta_range up to 1e4 lets theta pass 1e3, where edf is 1 and not the spline's value."""
    got, want, s1, _ = case_results("const_70x130_theta_1e4")
    models, cd, prior = make_inputs("const", 70, 130, True)
    assert np.sum(models["corr.theta"] > 1e3) > 40
    _, ref_edf = edf_tables()
    capped = R.moments(models, cd, ref_edf, s1["avmodes"], s1["matw"], theta_range=(1e-2, 1e3))
    assert np.max(np.abs(capped["edf"] / want["mom"]["edf"] - 1)) > 1e-4       # the branch matters here
    np.testing.assert_allclose(got["edf"], want["mom"]["edf"], rtol=1e-10)


def test_single_cell_level_joins_the_largest():
    got, want, _, _ = case_results("local_130x130_three_levels")
    assert sorted(set(got["batch"].tolist())) == ["a", "b"] and got["batch"][4] == "a"
    assert got["modes"].shape[0] == 2


def test_two_calls_return_the_same_bits():
    from scde_amd import varnorm as V
    case = "local_130x130_three_levels"
    got, _, s1, trend = case_results(case)
    models, cd, prior = make_inputs("local", 130, 130)
    batch, _ = _batch("three", 130)
    tab, _ = edf_tables()
    again = V.pagoda_varnorm(models, cd, tab, batch=batch, prior=prior, n_cores=1, n_randomizations=NRAND,
                             trend=trend, return_details=True)
    for k in ("mat", "matw", "arv", "edf", "wvar", "bwvar_ratio", "avmodes", "modes", "zval"):
        assert np.asarray(got[k]).tobytes() == np.asarray(again[k]).tobytes(), k


@pytest.mark.parametrize("case", ["local_70x37", "const_130x37_two_levels_power"])
def test_host_and_device_entries_agree_bit_for_bit(case):
    """The chain keeps the weights in HBM (the _dev entries); the _host entries take them from numpy."""
    from scde_amd import varnorm as V
    c = CASES[case]
    got, _, s1, _ = case_results(case)
    models, cd, prior = make_inputs(c["kind"], c["N"], c["C"])
    _, codes = _batch(c.get("batch"), c["C"])
    tab, _ = edf_tables()
    mom = V.varnorm_moments(models, cd, tab, s1["avmodes"], s1["matw"], s1["modes"], s1["bmatw"], codes,
                            weight_df_power=c.get("weight_df_power", 1))
    assert mom["edf"].tobytes() == got["edf"].tobytes()
    assert (mom["bwvar"] if codes is not None else mom["wvar"]).tobytes() == got["wvar"].tobytes()
    w = s1["bmatw"] if codes is not None else s1["matw"]
    mat, mw = V.varnorm_matrix(models, cd, w, got["arv"], codes, weight_k=0.9)
    assert mat.tobytes() == np.asfortranarray(got["mat"]).tobytes()
    assert mw.tobytes() == np.asfortranarray(got["matw"]).tobytes()


def test_zero_mode_gene_follows_ieee_rules():
    """avmodes = 0 gives lfpm = -inf; the kernel evaluates it like any other value, as R does."""
    from scde_amd import varnorm as V
    for kind in ("local", "const"):
        models, cd, prior = make_inputs(kind, 70, 37)
        tab, ref_edf = edf_tables()
        rng = np.random.default_rng(4)
        av = rng.uniform(0.5, 300, 70)
        av[[5, 64, 69]] = 0.0
        matw = rng.uniform(0.05, 1, cd.shape)
        got = V.varnorm_moments(models, cd, tab, av, matw)
        want = R.moments(models, cd, ref_edf, av, matw)
        for k in ("edf", "wvar", "rowsum_matw"):
            assert np.array_equal(np.isfinite(got[k]), np.isfinite(want[k])), k
            np.testing.assert_allclose(got[k], want[k], rtol=1e-10)


def test_built_in_smoother_end_to_end():
    from scde_amd import varnorm as V
    models, cd, prior = make_inputs("local", 130, 37)
    tab, ref_edf = edf_tables()
    got = V.pagoda_varnorm(models, cd, tab, prior=prior, n_cores=1, n_randomizations=NRAND, return_details=True,
                           minimize_underdispersion=True)
    v = got["vi"]
    assert v.sum() > 120 and np.isfinite(got["trend"][v]).all()
    assert np.isfinite(got["mat"][v]).all() and np.isfinite(got["arv"][v]).all()
    # the same trend fed back reproduces the run (the smoother is the only difference)
    again = V.pagoda_varnorm(models, cd, tab, prior=prior, n_cores=1, n_randomizations=NRAND, trend=got["trend"])
    assert again["mat"].tobytes() == got["mat"].tobytes()
    # zval scatters about 1 under its own trend
    assert 0.2 < np.median(got["zval"][v]) < 5
    # fit_genes: the trend is fitted on the subset's valid genes only, and predicted for every gene
    s1 = stage1(models, cd, prior, None)
    fit = list(range(0, 130, 2))
    sub = V.pagoda_varnorm(models, cd, tab, prior=prior, n_cores=1, n_randomizations=NRAND, return_details=True,
                           fit_genes=fit)
    fvi = sub["vi"].copy()
    fvi[1::2] = False
    with np.errstate(all="ignore"):
        lev, cv2 = np.log10(sub["avmodes"]), np.log10(sub["wvar"] / sub["avmodes"] ** 2)
    want = V.fit_trend(lev[fvi], cv2[fvi], weights=s1["matw"].sum(1)[fvi]).predict(lev)
    np.testing.assert_allclose(sub["trend"][sub["vi"]], want[sub["vi"]], rtol=1e-6, atol=1e-9)
    assert np.max(np.abs(sub["trend"][v] - V.pagoda_varnorm(
        models, cd, tab, prior=prior, n_cores=1, n_randomizations=NRAND, return_details=True)["trend"][v])) > 1e-6


def test_prior_none_calls_expression_prior():
    from scde_amd import varnorm as V
    from scde_amd.prior import expression_prior
    models, cd, _ = make_inputs("const", 70, 37)
    tab, _ = edf_tables()
    got = V.pagoda_varnorm(models, cd, tab, n_cores=1, n_randomizations=NRAND)
    want = expression_prior(models, cd, length_out=400)
    assert np.array_equal(got["prior"]["x"], want["x"]) and np.array_equal(got["prior"]["y"], want["y"])
    assert got["mat"].shape == cd.shape


def test_stages_refuse_weights_the_context_does_not_hold():
    from scde_amd import api
    from scde_amd._lib import ScdeError, check, lib
    from scde_amd.models import model_matrix
    models, cd, prior = make_inputs("const", 70, 37)
    stage1(models, cd[:64], prior, None)                   # the context now holds 64 x 37
    ctx = api.default_context()
    dc = api.DeviceCounts(ctx, cd)
    mm, lt, _ = model_matrix(models)
    tab, _ = edf_tables()
    out = np.zeros((3, 70))
    try:
        with pytest.raises(ScdeError, match="holds none of this shape"):
            check(lib().scde_pagoda_varnorm_moments_dev(ctx.handle, dc.ptr, 70, 70, 37, api._p(mm), lt, None, None,
                                                        None, None, 0, api._p(tab.table), tab.n, tab.lt0, tab.h,
                                                        1e-2, 1e2, 1.0, api._p(out)))
    finally:
        dc.free()


# ------------------------------------------------------------------ pagoda.subtract.aspect
def _aspect_inputs(N, C, seed):
    rng = np.random.default_rng(seed)
    mat = rng.normal(0, 2, (N, C)) + rng.normal(0, 1, (N, 1))
    matw = rng.uniform(0.02, 1.0, (N, C))
    aspect = rng.normal(0, 1, C) + 0.5 * mat[0]
    return mat, matw, aspect


@pytest.mark.parametrize("N,C", [(70, 37), (130, 130)])
@pytest.mark.parametrize("center", [True, False])
def test_subtract_aspect_matches_numpy(N, C, center):
    from scde_amd import varnorm as V
    mat, matw, aspect = _aspect_inputs(N, C, N + C)
    vi = {"mat": mat, "matw": matw, "arv": np.ones(N), "genes": [f"g{i}" for i in range(N)]}
    got = V.pagoda_subtract_aspect(vi, aspect, center=center)
    want = R.subtract_aspect(mat, matw, aspect, center)
    assert got["matw"] is matw and got["genes"] == vi["genes"] and vi["mat"] is mat
    # rtol from the issue; an element is a difference of terms up to max|mat| + |nr v| + |mean| in size, each
    # carrying a few roundings of its own sums (at most 130 terms): the absolute floor is 64 eps times that
    scale = np.abs(mat).max() * 3
    np.testing.assert_allclose(got["mat"], want, rtol=1e-12, atol=64 * np.finfo(float).eps * scale)
    v = aspect - aspect.mean()
    v /= np.sqrt((v ** 2).sum())
    if not center:
        proj = (got["mat"] * matw * v[None, :]).sum(1)
        size = np.abs(got["mat"] * matw * v[None, :]).sum(1)
        assert np.max(np.abs(proj) / size) < 1e-12
    else:
        assert np.max(np.abs((got["mat"] * matw).sum(1)) / np.abs(got["mat"] * matw).sum(1)) < 1e-12
    again = V.pagoda_subtract_aspect(vi, aspect, center=center)
    assert again["mat"].tobytes() == got["mat"].tobytes()
    with pytest.raises(ValueError):
        V.pagoda_subtract_aspect(vi, aspect[:-1])


# ------------------------------------------------------------------ the chain
def test_varinfo_feeds_the_downstream_functions():
    from scde_amd import pagoda_cluster_cells
    from scde_amd import varnorm as V
    from scde_amd.pagoda import pagoda_pathway_wPCA
    models, cd, prior = make_inputs("const", 130, 40)
    genes = [f"g{i}" for i in range(130)]
    import pandas as pd
    counts = pd.DataFrame(cd, index=genes, columns=[f"c{i}" for i in range(40)])
    tab, _ = edf_tables()
    vi = V.pagoda_varnorm(models, counts, tab, prior=prior, n_cores=1, n_randomizations=NRAND)
    assert vi["genes"] == genes and set(vi) >= {"mat", "matw", "arv", "modes", "avmodes", "prior", "edf", "batch",
                                                "trim"}
    setenv = {"setA": genes[10:40], "setB": genes[35:80], "setC": genes[80:125]}
    pw = pagoda_pathway_wPCA(vi, setenv, n_components=1, n_randomizations=3, n_starts=3)
    assert sorted(pw) == ["setA", "setB", "setC"]
    for r in pw.values():
        assert np.isfinite(r["xv"]).all() and np.isfinite(r["xp"]["scores"]).all() and r["n"] >= 20
    sub = V.pagoda_subtract_aspect(vi, pw["setA"]["xp"]["scores"][:, 0])
    ok = ~np.isnan(vi["mat"]).any(1)
    assert np.isfinite(sub["mat"][ok]).all()
    res = pagoda_cluster_cells({"gw": {g: 1.0 for g in genes}}, sub, min_overdispersion=0, return_details=True)
    assert len(res["genes"]) > 50
    assert np.isfinite(res["clustering"].height).all() and len(res["clustering"].order) == 40
