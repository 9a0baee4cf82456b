"""GPU tests of pagoda.top.aspects' matrix step (csrc/top_aspects.hip) and of the route from
pagoda_pathway_wPCA to the cell embedding through pagoda_top_aspects.

The tolerance rule is the one of tests/test_gpu_aspects.py: the GPU's maximum error against
np.longdouble is at most 16 x the float64 restatement's own maximum error on the same case plus
8 ulp of the result's scale, and NaN appears exactly where the restatement has it.  Every test
prints the figures before it asserts.
"""
import ctypes

import numpy as np
import pytest

import top_aspects_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (3, 63), (3, 64), (3, 65), (70, 257), (5, 1000)]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def make_case(m, c, seed=0):
    """x, w (m x c).  With three rows or more: row 0 constant (a value whose sums are exact, so
    every summation order leaves a variance of exactly 0), row 1 of magnitude 1e150, weight row 2
    summing to a subnormal number."""
    rng = np.random.default_rng(1000 * m + c + seed)
    x = rng.normal(size=(m, c)) * rng.uniform(0.1, 10.0, size=(m, 1)) + rng.normal(size=(m, 1))
    w = rng.uniform(0.05, 1.0, size=(m, c))
    if m >= 3:
        x[0] = -2.5
        x[1] = 1e150 * rng.normal(size=c)
        w[2] = 5e-324 * rng.integers(1, 40, size=c)
    return x, w


def nums(m, mode, seed=0):
    rng = np.random.default_rng(77 + m + seed)
    # the chi-squared factor sqrt(qchisq(.) / n.cells) is near 1; a score var / exp spreads wider
    return rng.uniform(0.9, 1.6, size=m) if mode == "chisq" else rng.uniform(0.4, 30.0, size=m)


def host_entry(x, w, num):
    from scde_amd import api
    from scde_amd._lib import check, lib
    m, c = x.shape
    xv, xvw = np.full((m, c), 7.0), np.full((m, c), 7.0)
    check(lib().scde_top_aspects(api.default_context().handle, api._p(x), api._p(w), api._p(num), m, c, api._p(xv),
                                 api._p(xvw)))
    return xv, xvw


def dev_entry(x, w, num):
    from scde_amd import api, aspects
    from scde_amd._lib import check
    m, c = x.shape
    dev = aspects._Dev(api.default_context())
    try:
        xd, wd = dev.put(x), dev.put(w)
        vd, od = dev.alloc(x.nbytes), dev.alloc(x.nbytes)
        check(dev.L.scde_top_aspects_dev(dev.ctx.handle, xd, wd, api._p(num), m, c, vd, od))
        return dev.get(vd, (m, c), "C"), dev.get(od, (m, c), "C")
    finally:
        dev.free()


def check_rule(got, exact, ref64, what):
    got, ref64, exact = np.asarray(got, np.float64), np.asarray(ref64, np.float64), np.asarray(exact)
    nan = np.isnan(ref64)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs from the restatement's"
    ok = ~nan
    if not ok.any():
        return
    e_gpu = float(np.abs(got.astype(np.longdouble) - exact)[ok].max())
    e_ref = float(np.abs(ref64.astype(np.longdouble) - exact)[ok].max())
    scale = float(np.abs(exact[ok]).max())
    print(f"{what}: gpu max err {e_gpu:.3g}, restatement's own {e_ref:.3g}, bar {R.bar(e_ref, scale):.3g}")
    assert e_gpu <= R.bar(e_ref, scale), (what, e_gpu, e_ref, scale)


@pytest.mark.parametrize("mode", ["chisq", "oe"])
@pytest.mark.parametrize("m,c", SHAPES)
def test_device_stage_against_restatement(m, c, mode):
    x, w = make_case(m, c)
    num = nums(m, mode)
    xv, xvw = host_entry(x, w, num)
    r_xv, r_xvw = R.scale_rows(x, w, num)
    e_xv, e_xvw = R.scale_rows(x, w, num, dtype=np.longdouble)
    if m >= 3:
        assert np.all(np.isnan(r_xv[0])) and np.all(np.isfinite(r_xv[1:]))     # the constant row: 0 * Inf
    # per row: the rows' factors differ by orders of magnitude in "oe" mode
    for r in range(m):
        check_rule(xv[r], e_xv[r], r_xv[r], f"xv {m}x{c} {mode} row {r}")
        check_rule(xvw[r], e_xvw[r], r_xvw[r], f"xvw {m}x{c} {mode} row {r}")
    ok = ~np.isnan(xv).any(axis=1)
    assert np.all(np.abs(xv[ok].mean(axis=1)) <= 64 * R.U * np.abs(xv[ok]).max(axis=1))
    assert np.allclose(xv[ok].std(axis=1, ddof=1), num[ok], rtol=1e-13)
    assert np.allclose(xvw.sum(axis=1), 1.0, rtol=1e-13)


@pytest.mark.parametrize("m,c", [(3, 64), (4, 1003), (70, 257)])
def test_bit_equality(m, c):
    """Two runs give the same bits, and so do the host and the device entry; with c = 1003 every
    other row starts off a 16-byte boundary and the last cell is the unpaired one."""
    x, w = make_case(m, c, seed=1)
    num = nums(m, "chisq", seed=1)
    a = host_entry(x, w, num)
    b = host_entry(x, w, num)
    d = dev_entry(x, w, num)
    for k, what in enumerate(("xv", "xvw")):
        assert np.array_equal(bits(a[k]), bits(b[k])), what
        assert np.array_equal(bits(a[k]), bits(d[k])), what
    r_xv, r_xvw = R.scale_rows(x, w, num)
    e_xv, e_xvw = R.scale_rows(x, w, num, dtype=np.longdouble)
    for r in range(m):
        check_rule(d[0][r], e_xv[r], r_xv[r], f"xv {m}x{c} row {r}")
        check_rule(d[1][r], e_xvw[r], r_xvw[r], f"xvw {m}x{c} row {r}")


def test_argument_errors_and_empty():
    from scde_amd import api
    from scde_amd._lib import ScdeError, check, lib
    x = np.ones((2, 3))
    out = np.zeros((2, 3))
    h = api.default_context().handle
    with pytest.raises(ScdeError, match="bad dimensions"):
        check(lib().scde_top_aspects(h, api._p(x), api._p(x), api._p(x), 2, 0, api._p(out), api._p(out)))
    with pytest.raises(ScdeError, match="null argument"):
        check(lib().scde_top_aspects(h, None, api._p(x), api._p(x), 2, 3, api._p(out), api._p(out)))
    check(lib().scde_top_aspects(h, None, None, None, 0, 3, None, None))   # no rows: nothing to do
    check(lib().scde_top_aspects_dev(h, None, None, None, 0, 3, None, None))
    assert ctypes.sizeof(ctypes.c_double) == 8


@pytest.mark.parametrize("oe", [False, True])
def test_top_aspects_both_scale_modes(oe):
    """pagoda_top_aspects on the hand-made pwpca / clpca of tests/test_top_aspects.py: the tam's
    rows, names and matrices against the restatement with the table's own factors."""
    from scipy.special import log_ndtr

    import test_top_aspects as H
    from scde_amd import top_aspects as T
    pw, cl = H.make_pwpca(), H.make_clpca()
    t = T.top_aspects_table(pw, cl, n_cells=H.CELLS)
    tam = T.pagoda_top_aspects(pw, cl, n_cells=H.CELLS, use_oe_scale=oe)
    rows = np.nonzero(t["valid"])[0]
    assert len(rows) >= 3 and tam["xv"].shape == (len(rows), H.CELLS) == tam["xvw"].shape
    assert tam["names"] == [f"#PC{t['npc'][r]}# {t['name'][r]}" for r in rows]
    assert "#PC1# set2" in tam["names"] and "#PC1# geneCluster.2" in tam["names"]
    x = np.array([t["sets"][t["i"][r] - 1][1]["xp"]["scores"][:, t["npc"][r] - 1] for r in rows])
    w = np.array([t["sets"][t["i"][r] - 1][1]["xp"]["scoreweights"][:, t["npc"][r] - 1] for r in rows])
    num = t["score"][rows] if oe else np.sqrt(T.qchisq_upper_log(log_ndtr(-t["z"][rows]), H.CELLS) / H.CELLS)
    r_xv, r_xvw = R.scale_rows(x, w, num)
    e_xv, e_xvw = R.scale_rows(x, w, num, dtype=np.longdouble)
    for r in range(len(rows)):
        check_rule(tam["xv"][r], e_xv[r], r_xv[r], f"tam xv row {r} oe={oe}")
        check_rule(tam["xvw"][r], e_xvw[r], r_xvw[r], f"tam xvw row {r} oe={oe}")
    assert tam["gw"] == T.pagoda_top_aspects(pw, cl, n_cells=H.CELLS, return_genes=True)
    assert len(tam["df"]) == len(t["var"]) and list(tam["df"]["name"]) == t["name"]


def test_route_to_the_embedding():
    """models-free end of the walkthrough on a synthetic varinfo: 600 genes x 120 cells, three
    planted modules of 30 genes that share a cell factor, unit weights; the gene sets are the
    modules and 20 random sets.  Every stage takes the previous one's output unchanged."""
    import scde_amd as S
    rng = np.random.default_rng(11)
    ngenes, ncells = 600, 120
    mat = rng.normal(size=(ngenes, ncells))
    for k in range(3):
        factor = rng.normal(size=ncells)
        mat[30 * k:30 * (k + 1)] += 1.2 * factor * rng.choice([-1.0, 1.0], size=(30, 1))
    # bwpca's variances are weighted sums over the cells: with unit weights a null gene has to
    # sum to 1 over its cells (what pagoda.varnorm's scaling gives) for the Wishart null to apply
    mat /= np.sqrt(ncells)
    genes = [f"g{i}" for i in range(ngenes)]
    varinfo = {"mat": mat, "matw": np.ones_like(mat), "batch": None, "genes": genes, "arv": np.full(ngenes, 1.0)}
    setenv = {f"module{k}": genes[30 * k:30 * (k + 1)] for k in range(3)}
    for k in range(20):
        setenv[f"random{k}"] = [genes[i] for i in rng.choice(np.arange(90, ngenes), size=30, replace=False)]
    from scde_amd.pagoda import pagoda_pathway_wPCA
    pw = pagoda_pathway_wPCA(varinfo, setenv, n_components=1, n_randomizations=10)
    cl = S.pagoda_gene_clusters(varinfo, n_clusters=12, n_samples=6)
    df = S.pagoda_top_aspects(pw, cl, return_table=True)
    tam = S.pagoda_top_aspects(pw, cl)
    print(df.to_string())
    valid = set(tam["names"])
    assert {f"#PC1# module{k}" for k in range(3)} <= valid
    assert any(f"#PC1# random{k}" not in valid for k in range(20))
    assert len(df) == len(tam["names"]) and np.all(np.isfinite(tam["xv"])) and np.all(np.isfinite(tam["xvw"]))
    tamr = S.pagoda_reduce_loading_redundancy(tam, pw, cl)
    tamr2 = S.pagoda_reduce_redundancy(tamr)
    assert 1 <= len(tamr2["names"]) <= len(tamr["names"]) <= len(tam["names"])
    assert set(tamr2) >= {"xv", "xvw", "names", "cnam", "gw", "df"}
    det = S.pagoda_cluster_cells(tamr2, varinfo, return_details=True)
    Y = np.asarray(S.tsne_embedding(det["distance"], perplexity=10, max_iter=50))
    assert Y.shape == (ncells, 2) and np.all(np.isfinite(Y))
