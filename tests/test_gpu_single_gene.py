"""``scde_test_gene_expression_difference`` on the DE walkthrough's data (Darwin rand), against
R's printed lines (vignettes/diffexp.md:138-139 and 166-167) and against the oracle.

The walkthrough's ``batch`` is ``rbinom(40, 1, 0.5)`` after ``set.seed(1)``: one uniform per cell,
1 when u >= 0.5 (R's inversion branch for n * p < 30).  The vector rebuilt that way gives the
printed group-by-batch table (11 9 / 8 12), and the oracle with it reproduces the printed batch
line, so the GPU is pinned to that line at the precision of the print."""
import numpy as np
import pytest

from conftest import assert_posterior_close, assert_z_close, golden
from test_oracle import VIGNETTE_TDH_SINGLE

pytestmark = pytest.mark.gpu

# vignettes/diffexp.md:166-167 (scde.test.gene.expression.difference("Tdh", batch = batch))
VIGNETTE_TDH_BATCH = (3.659705, 7.796764, 12.01338, 3.659705, 3.782082, 3.782082)
COLS = ["lb", "mle", "ub", "ce", "Z", "cZ"]


@pytest.fixture(scope="module")
def api():
    from scde_amd import api
    return api


@pytest.fixture(scope="module")
def inputs():
    import pandas as pd
    from oracle.oracle import MODEL_COLUMNS
    v = golden("esmef_vignette_inputs.npz")
    md = {c: v["models"][:, j] for j, c in enumerate(MODEL_COLUMNS) if not np.all(np.isnan(v["models"][:, j]))}
    cells = list(v["cells"])
    # only the rows the tests name travel to the device
    keep = [list(v["genes"]).index(g) for g in ("Tdh", "Dppa5a")]
    counts = pd.DataFrame(v["counts"][keep], index=["Tdh", "Dppa5a"], columns=cells)
    groups = pd.Series(pd.Categorical(np.where(v["groups"] == 0, "ESC", "MEF"), categories=["ESC", "MEF"]),
                       index=cells)
    prior = {"x": v["prior_x"], "y": v["prior_y"]}
    return dict(v=v, md=md, models=pd.DataFrame(md, index=cells), counts=counts, groups=groups, prior=prior)


@pytest.fixture(scope="module")
def batch(inputs):
    from scde_amd import api
    from scde_amd._lib import check, lib
    n = len(inputs["groups"])
    state, u = np.zeros(625, np.uint32), np.zeros(n)
    check(lib().scde_r_set_seed(1, api._p(state)))
    check(lib().scde_r_unif_rand(api._p(state), n, api._p(u)))
    b = np.where(u >= 0.5, "batch1", "batch2")
    g = inputs["v"]["groups"]
    assert [[int(np.sum((g == k) & (b == lv))) for lv in ("batch1", "batch2")] for k in (0, 1)] == [[11, 9], [8, 12]]
    return list(b)


@pytest.fixture()
def darwin(api, oracle):
    api.set_rand("darwin")
    oracle.set_rng(2)
    yield
    api.set_rand("glibc")
    oracle.set_rng(0)


def row(table):
    return table.loc["Tdh", COLS].to_numpy(dtype=float)


def test_tdh_without_batch(api, oracle, inputs, darwin):
    got = api.scde_test_gene_expression_difference("Tdh", inputs["models"], inputs["counts"], inputs["prior"],
                                                    groups=inputs["groups"])
    print("GPU      ", row(got), "\nR prints ", VIGNETTE_TDH_SINGLE)
    np.testing.assert_allclose(row(got), VIGNETTE_TDH_SINGLE, atol=6e-6, rtol=0)
    v = inputs["v"]
    ref = oracle.scde_expression_difference(inputs["md"], inputs["counts"].loc[["Tdh"]].to_numpy(), v["prior_x"],
                                            v["prior_y"], v["groups"], n_randomizations=1000, n_cores=1,
                                            return_posteriors=True)
    for k in ("lb", "mle", "ub", "ce"):
        np.testing.assert_array_equal(got[k].to_numpy(), ref["results"][k], err_msg=k)
    assert_z_close(got["Z"].to_numpy(), ref["results"]["Z"])
    assert_z_close(got["cZ"].to_numpy(), ref["results"]["cZ"], what="cZ")
    # the detailed return
    det = api.scde_test_gene_expression_difference("Tdh", inputs["models"], inputs["counts"], inputs["prior"],
                                                    groups=inputs["groups"], return_details=True)
    assert set(det) == {"results", "difference.posterior", "posteriors"}
    np.testing.assert_array_equal(row(det["results"]), row(got))
    assert list(det["posteriors"]) == ["ESC", "MEF"]
    G = len(v["prior_x"])
    assert det["difference.posterior"].values.shape == (1, 2 * G - 1)
    for k, lv in enumerate(("ESC", "MEF")):
        p = det["posteriors"][lv]
        assert_posterior_close(p["jp"], ref["joint.posteriors"][k], what=f"jp {lv}")
        assert len(p["post"]) == 20 and p["post"][0].shape == (1, G)


def test_tdh_with_batch(api, oracle, inputs, batch, darwin):
    det = api.scde_test_gene_expression_difference("Tdh", inputs["models"], inputs["counts"], inputs["prior"],
                                                    groups=inputs["groups"], batch=batch, return_details=True)
    assert set(det) == {"results", "difference.posterior", "results.nobatchcorrection"}
    print("GPU      ", row(det["results"]), "\nR prints ", VIGNETTE_TDH_BATCH)
    np.testing.assert_allclose(row(det["results"]), VIGNETTE_TDH_BATCH, atol=6e-6, rtol=0)
    np.testing.assert_allclose(row(det["results.nobatchcorrection"]), VIGNETTE_TDH_SINGLE, atol=6e-6, rtol=0)
    v = inputs["v"]
    ref = oracle.scde_expression_difference_batch(inputs["md"], inputs["counts"].loc[["Tdh"]].to_numpy(),
                                                  v["prior_x"], v["prior_y"], v["groups"], batch,
                                                  n_randomizations=1000, n_cores=1)
    for name, key in (("results", "batch.adjusted"), ("results.nobatchcorrection", "results")):
        for k in ("lb", "mle", "ub", "ce"):
            np.testing.assert_array_equal(det[name][k].to_numpy(), ref[key][k], err_msg=f"{name} {k}")
        assert_z_close(det[name]["Z"].to_numpy(), ref[key]["Z"], what=f"{name} Z")
    G = len(v["prior_x"])
    assert det["difference.posterior"].values.shape == (1, 4 * G - 3)
    # the plain return is the adjusted table; one batch level is no correction
    got = api.scde_test_gene_expression_difference("Tdh", inputs["models"], inputs["counts"], inputs["prior"],
                                                    groups=inputs["groups"], batch=batch)
    np.testing.assert_array_equal(row(got), row(det["results"]))
    one = api.scde_test_gene_expression_difference("Tdh", inputs["models"], inputs["counts"], inputs["prior"],
                                                    groups=inputs["groups"], batch=["b"] * len(batch))
    np.testing.assert_array_equal(row(one), row(det["results.nobatchcorrection"]))


def test_errors(api, inputs):
    m, c, p, g = inputs["models"], inputs["counts"], inputs["prior"], inputs["groups"]
    with pytest.raises(ValueError, match=r"specified gene \(NoSuchGene\) is not found in the count data"):
        api.scde_test_gene_expression_difference("NoSuchGene", m, c, p, groups=g)
    with pytest.raises(ValueError, match="wrong number of levels in the grouping factor"):
        api.scde_test_gene_expression_difference("Tdh", m, c, p, groups=["ESC"] * len(g))
    with pytest.raises(ValueError, match="groups factor is not provided"):
        api.scde_test_gene_expression_difference("Tdh", m, c, p)
