"""GPU tests of scde_amd/views.py against the numpy restatement in tests/views_ref.py, on the
synthetic case tests/test_views.py establishes (its selection gaps make the discrete results --
the genes kept, both trees -- independent of a rounding).  Discrete results are equal; values are
compared with the tolerance tests/test_gpu_wpca.py uses for ``xv`` (rtol 1e-6, atol 1e-9)."""
import math
import warnings

import numpy as np
import pytest

import views_ref as V

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol=1e-9)
GIVEN = "a tree from elsewhere"  # passed through untouched by both sides


@pytest.fixture(scope="module")
def S():
    from scde_amd import views
    return views


@pytest.fixture(scope="module")
def case():
    return V.make_case()


def same_tree(got, ref, what):
    merge, _, order = ref
    assert np.array_equal(got.merge, merge), f"{what}: merge differs"
    assert np.array_equal(got.order, order), f"{what}: order differs"


def compare(got, ref, what):
    assert (got is None) == (ref is None), what
    if ref is None:
        return
    assert list(got["lab"]) == list(ref["lab"]), f"{what}: lab"
    assert np.array_equal(got["row_order"], ref["row_order"]), f"{what}: row_order"
    assert got.get("consensus_pc") == ref.get("consensus_pc"), what
    assert (got["hc"] is None) == (ref["hc"] is None)
    if ref["hc"] is not None:
        same_tree(got["hc"], ref["hc"], f"{what}: gene tree")
    if ref["vhc"] is GIVEN:
        assert got["vhc"] is GIVEN
    else:
        same_tree(got["vhc"], ref["vhc"], f"{what}: cell tree")
    keys = ["vmap", "zlim", "aval"] + (["oc", "scores", "rotation", "sd"] if "scores" in ref else [])
    assert ("scores" in got) == ("scores" in ref)
    for k in keys:
        np.testing.assert_allclose(np.asarray(got[k]), np.asarray(ref[k]), err_msg=f"{what}: {k}", **TOL)


SHOW_CASES = {
    "several": dict(pathways=["GO:A", "GO:B"]),
    "several two-sided": dict(pathways=["GO:A", "GO:B"], two_sided=True),
    "several, the other way round": dict(pathways=["GO:B", "GO:A"], n_genes=11),
    "several trimmed": dict(pathways=["GO:A", "GO:B"], trim=2.1 / V.C),
    "fewer than 3": dict(pathways=["GO:A", "GO:B"], n_genes=2),
    "one": dict(pathways=["GO:A"], n_genes=12),
    "one, all genes": dict(pathways=["GO:A"], n_genes=100),
    "one, second component": dict(pathways=["GO:B"], n_genes=12, n_pc=[2]),
    "genes": dict(pathways=V.SET_A[:15]),
    # (over two genes every cell-to-cell correlation is +-1 or NaN: the cell tree is all ties, so it is given)
    "two genes": dict(pathways=["g1", "g2"], cell_clustering=GIVEN),
    "given zlim": dict(pathways=["GO:A"], zlim=(-0.5, 0.7)),
}


@pytest.mark.parametrize("name", list(SHOW_CASES))
def test_show_pathways(S, case, name):
    varinfo, goenv, _ = case
    kw = dict(SHOW_CASES[name])
    pathways = kw.pop("pathways")
    ref = V.show_pathways(pathways, varinfo, goenv, **kw)
    got = S.pagoda_show_pathways(pathways, varinfo, goenv, return_details=True, **kw)
    compare(got, ref, name)
    plain = S.pagoda_show_pathways(pathways, varinfo, goenv, **kw)
    if ref is None:
        assert plain is None
    else:
        assert np.array_equal(plain, got["scores"][:, 0])


def test_show_pathways_given_cell_clustering(S, case):
    varinfo, goenv, _ = case
    from scde_amd import cluster
    hc = cluster.hclust_dist(np.asarray(varinfo["mat"]).T[:, :10])
    got = S.pagoda_show_pathways(["GO:A"], varinfo, goenv, cell_clustering=hc, return_details=True)
    assert got["vhc"] is hc


def test_show_pathways_with_device_is_bit_identical(S, case):
    from scde_amd.pagoda import PagodaDevice
    varinfo, goenv, _ = case
    dev = PagodaDevice(varinfo)
    try:
        for name in ("several", "several two-sided", "one", "one, second component", "genes"):
            kw = dict(SHOW_CASES[name])
            pathways = kw.pop("pathways")
            a = S.pagoda_show_pathways(pathways, varinfo, goenv, return_details=True, **kw)
            b = S.pagoda_show_pathways(pathways, varinfo, goenv, return_details=True, device=dev, **kw)
            assert a["lab"] == b["lab"]
            for k in ("oc", "scores", "rotation", "vmap", "aval", "sd", "var"):
                assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (name, k)
            for t in ("hc", "vhc"):
                assert np.array_equal(a[t].merge, b[t].merge) and np.array_equal(a[t].height, b[t].height)
        with pytest.raises(ValueError, match="trim must be 0"):
            S.pagoda_show_pathways(["GO:A"], varinfo, goenv, device=dev, trim=0.1)
    finally:
        dev.free()


def test_show_pathways_names(S, case):
    varinfo, goenv, _ = case
    with pytest.warns(UserWarning, match="partial match to pathway names.*GO:nope"):
        got = S.pagoda_show_pathways(["GO:A", "GO:nope"], varinfo, goenv, n_genes=12)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ref = S.pagoda_show_pathways(["GO:A"], varinfo, goenv, n_genes=12)
    assert np.array_equal(got, ref)
    with pytest.warns(UserWarning, match="partial match to gene names.*nope"):
        S.pagoda_show_pathways(["g1", "g2", "g3", "nope"], varinfo, goenv)
    with pytest.raises(ValueError, match="do not match either gene nor pathway names"):
        S.pagoda_show_pathways(["nothing"], varinfo, goenv)


def test_pattern_feeds_subtract_aspect(S, case):
    """The walkthrough's last step on the device: the planted sets' PC1 sd drops."""
    from scde_amd import pagoda as PG
    from scde_amd.varnorm import pagoda_subtract_aspect
    varinfo, goenv, _ = case
    pattern = S.pagoda_show_pathways(["GO:A", "GO:B"], varinfo, goenv)
    kw = dict(n_components=1, min_pathway_size=0, n_randomizations=0, n_starts=2)
    before = PG.pagoda_pathway_wPCA(varinfo, goenv, **kw)
    after = PG.pagoda_pathway_wPCA(pagoda_subtract_aspect(varinfo, pattern), goenv, **kw)
    for p in ("GO:A", "GO:B"):
        assert after[p]["sd"][0, 0] < before[p]["sd"][0, 0]


@pytest.mark.parametrize("names,kw", [(["GO:A"], {}), (["GO:A", "GO:C"], dict(n_pc=2)),
                                      (["g3", "g1"], dict(cell_clustering=GIVEN)),
                                      (["g7", "g3", "g1", "g60"], dict(trim=0)), (["GO:B"], dict(zlim=(-1.0, 1.0)))])
def test_view_pathway_genes(S, case, names, kw):
    varinfo, goenv, _ = case
    ref = V.pathway_genes(names, varinfo, goenv, **kw)
    got = S.view_pathway_genes(names, varinfo, goenv, **kw)
    compare(got, ref, str(names))
    assert got["lab_names"] == ref["lab_names"]
    if "oc" in got:
        assert V.spearman(got["oc"], got["aval"]) >= 0
    assert S.view_pathway_genes(["nothing"], varinfo, goenv) is None


@pytest.fixture(scope="module")
def tamr():
    rng = np.random.default_rng(3)
    xv = rng.normal(size=(7, 40)) * np.array([1, 5, 2, 5, 3, 0.5, 4])[:, None]
    return {"xv": xv, "xvw": np.abs(xv) + 1, "cnam": [[f"a{i}"] for i in range(7)]}


@pytest.mark.parametrize("top", [math.inf, 1, 3, 7, 100])
def test_view_aspects(S, tamr, top):
    from scde_amd import cluster
    ref = V.view_aspects(tamr["xv"], top)
    got = S.pagoda_view_aspects(tamr, top=top)
    assert np.array_equal(got["xv"], tamr["xv"][ref["vi"]]) and np.array_equal(got["xvw"], tamr["xvw"][ref["vi"]])
    assert list(got["cnam"]) == [tamr["cnam"][i] for i in ref["vi"]]
    assert np.array_equal(got["rcmvar"], ref["rcmvar"])
    assert got["zlim"] == ref["zlim"] and np.array_equal(got["mat"], ref["mat"])
    if ref["row_clustering"] is None:
        assert got["row_clustering"] is None
        return
    same_tree(got["row_clustering"], ref["row_clustering"], f"top={top}")
    # the tree is hclust(dist(.)) of the rows kept
    hc = cluster.hclust(cluster.dist(got["xv"]), "complete")
    assert np.array_equal(got["row_clustering"].merge, hc.merge)
    assert np.array_equal(got["row_clustering"].height, hc.height)
    given = S.pagoda_view_aspects(tamr, row_clustering=hc, top=top)
    assert given["row_clustering"] is hc
