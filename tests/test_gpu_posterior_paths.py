"""Branches of the posterior's host path (run_posterior, scde_amd/csrc/engine_posterior.hip) that
no other test reaches, against the CPU oracle (SURVEY.md §8(d) tolerance) and the `boot_path` stat:

* the host packing of the byte multiplicities -- above 16,384 cells the multiplicity arrays are
  formed on the host, not by the device kernel -- on the tile path and on the stretch path;
* the general bootstrap kernel (grids above 1,024 points);
* the split of a posterior into its tables and the rest, which the two-lane DE call uses to
  queue both groups' tables before either bootstrap.
"""
import numpy as np
import pytest

from conftest import assert_cz_close, assert_posterior_close, assert_z_close, golden

pytestmark = pytest.mark.gpu

MULT_MAX_CELLS = 16384  # kMultMaxCells (kernels.h): the device forms the multiplicities up to here


@pytest.fixture(scope="module")
def api():
    from scde_amd import api as A
    A.set_rand("glibc")
    return A


def _models(g):
    from oracle.oracle import MODEL_COLUMNS
    m = g["models"]
    return {c: m[:, j] for j, c in enumerate(MODEL_COLUMNS) if not np.all(np.isnan(m[:, j]))}


def test_host_multiplicities_tiles_and_stretch(api, oracle):
    """16,385 cells, one more than the device multiplicity kernel takes: W, w8, w8t and w8g are
    packed on the host.  Default options take the tile path (boot_path 1), boot_tiles = 0 the
    stretch path (boot_path 0); both match the oracle and give the same bits."""
    g = golden("esmef500.npz")
    C, N = MULT_MAX_CELLS + 1, 4
    rng = np.random.default_rng(5)
    models = _models(g)
    rows = rng.integers(0, len(next(iter(models.values()))), C)
    mm, lt, sq = oracle.model_matrix({k: v[rows] for k, v in models.items()})
    counts = rng.poisson(0.7, (N, C)).astype(np.int32)
    counts[0] = 0
    ucl, uci = oracle.ucl_uci(counts)
    mag = oracle.marginals_from_prior_x(g["prior_x"])
    assert mag.shape[0] == 401
    ref = oracle.logBootPosterior(mm, ucl, uci, mag, 3, 7, 0, lt, sq, 0)
    assert np.isfinite(ref).all()  # the comparison leaves no row out
    ctx = api.default_context()
    got = {}
    try:
        for name, tiles, path in (("tiles", 1, 1), ("stretch", 0, 0)):
            ctx.set_option("boot_tiles", tiles)
            api.set_rand("glibc")
            got[name] = api.logBootPosterior(mm, ucl, uci, mag, 3, 7, 0, lt, sq, 0, ctx=ctx)
            assert ctx.stat("boot_path") == path, (name, ctx.stat("boot_path"))
            assert_posterior_close(got[name], ref, what=f"jp {name}")
    finally:
        ctx.set_option("boot_tiles", 1)
    np.testing.assert_array_equal(got["tiles"], got["stretch"])


def test_general_bootstrap_path(api, oracle):
    """The 1,201-point grid of test_gpu_parity.py's test_expression_difference_grid_sizes: more than
    1,024 lanes, so the general kernel k_boot runs (boot_path 3)."""
    from scde_amd.prior import expression_prior
    g = golden("esmef500.npz")
    models = _models(g)
    counts = np.ascontiguousarray(g["counts"][:70])
    prior = expression_prior(models, counts, length_out=1200)
    api.set_rand("glibc")
    got = api.scde_expression_difference(models, counts, prior, groups=list(g["groups"]), n_randomizations=10,
                                         n_cores=2, return_posteriors=True)
    assert api.default_context().stat("boot_path") == 3
    ref = oracle.scde_expression_difference(models, counts, prior["x"], prior["y"], g["groups"], n_randomizations=10,
                                            n_cores=2, return_posteriors=True)
    for i in range(2):
        assert_posterior_close(got["joint.posteriors"][i], ref["joint.posteriors"][i], what=f"jp{i}")
    assert_posterior_close(got["difference.posterior"].values, ref["difference.posterior"], what="ratio")
    res = got["results"]
    for k in ("lb", "mle", "ub", "ce"):
        np.testing.assert_array_equal(res[k].to_numpy(), ref["results"][k], err_msg=k)
    assert_z_close(res["Z"].to_numpy(), ref["results"]["Z"])
    assert_cz_close(res["cZ"].to_numpy(), ref["results"]["cZ"], res["Z"].to_numpy(), ref["results"]["Z"])


def test_tables_first_split_equals_one_lane(api):
    """The first 256 genes of the config 3 fixture's data set: with lanes = 2 the DE call queues
    both groups' tables before either group's bootstrap (run_posterior's `rest`), with lanes = 1
    each posterior runs whole.  Same bits in every output."""
    import bench
    g = golden("config3_full.npz")
    seed, ngenes, ncells, nboot, ncores = (int(v) for v in g["meta"])
    models, counts, groups = bench.synthetic(seed, ngenes, ncells, two_groups=True)
    counts = np.ascontiguousarray(counts[:256])
    prior = {"x": g["prior_x"], "y": g["prior_y"]}
    ctx = api.default_context()
    got = {}
    try:
        for lanes in (2, 1):
            ctx.set_option("lanes", lanes)
            api.set_rand("glibc")
            got[lanes] = api.scde_expression_difference(models, counts, prior, groups=list(groups),
                                                        n_randomizations=nboot, n_cores=ncores,
                                                        return_posteriors=True)
    finally:
        ctx.set_option("lanes", 2)
    a, b = got[2], got[1]
    assert np.isfinite(a["results"][["lb", "mle", "ub", "ce"]].to_numpy()).all()
    np.testing.assert_array_equal(a["results"].to_numpy(), b["results"].to_numpy())
    for i in range(2):
        np.testing.assert_array_equal(a["joint.posteriors"][i], b["joint.posteriors"][i], err_msg=f"jp{i}")
    np.testing.assert_array_equal(a["difference.posterior"].values, b["difference.posterior"].values)
