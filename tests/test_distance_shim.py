"""The distance measures' .Call entries (R/src/scde_hip_shim.c: scde_hip_reciprocal_corr,
scde_hip_mode_fail_corr, scde_hip_direct_corr) through the R-API stand-in of
tests/test_shim_minir.py: R-shaped arguments in, the Python mirror's values out."""
import numpy as np
import pytest

from conftest import golden, gpu_available

minir = pytest.importorskip("minir")


@pytest.fixture(scope="module")
def shim():
    import os
    if not os.path.exists(minir.SO):
        minir.build()
    minir.lib()
    return minir


def _inputs():
    from scde_amd.models import model_matrix
    from test_distance import _fixture
    g, models, cd = _fixture("knn300.npz", np.arange(50), np.arange(20))
    mm, _, sq = model_matrix(models)
    return g, models, np.asfortranarray(cd, np.int32), mm, sq


def test_shim_distance_argument_errors_are_rf_error(shim):
    _, _, cd, mm, sq = _inputs()
    with pytest.raises(shim.RError, match="models and counts disagree"):
        shim.call("scde_hip_reciprocal_corr", mm[:7], cd, bool(sq), 0.95)
    with pytest.raises(shim.RError, match="k must be in"):
        shim.call("scde_hip_reciprocal_corr", mm, cd, bool(sq), 1.5)
    with pytest.raises(shim.RError, match="uniforms must hold"):
        shim.call("scde_hip_direct_corr", mm, cd, bool(sq), 0.9, 2, np.zeros(5), 1.0)
    with pytest.raises(shim.RError, match="nsim must be"):
        shim.call("scde_hip_direct_corr", mm, cd, bool(sq), 0.9, 0, None, 1.0)
    with pytest.raises(shim.RError, match="modes must be genes x cells"):
        shim.call("scde_hip_mode_fail_corr", mm, cd, bool(sq), np.zeros((50, 19)), np.zeros(50))


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU error path")
def test_shim_distance_no_gpu_is_rf_error(shim):
    _, _, cd, mm, sq = _inputs()
    with pytest.raises(shim.RError, match="scde_hip: .*device"):
        shim.call("scde_hip_reciprocal_corr", mm, cd, bool(sq), 0.95)


@pytest.mark.gpu
def test_shim_distance_entries_match_python(shim):
    from scde_amd import direct_dropout_distance, mode_relative_distance, reciprocal_distance
    from scde_amd.distance import joint_posterior_modes
    g, models, cd, mm, sq = _inputs()
    off = ~np.eye(20, dtype=bool)  # the Python API zeroes the distance's diagonal
    # R passes counts as an integer matrix, flags as logicals, k / n.simulations / seed as doubles
    got = shim.call("scde_hip_reciprocal_corr", mm, cd, bool(sq), 0.95)
    assert got.shape == (20, 20)
    assert np.array_equal((1 - got)[off], reciprocal_distance(models, cd, k=0.95)[off])
    modes = np.asfortranarray(golden("knn300.npz")["modes"][:50, :20])
    jp = g["jp"][:50]
    got = shim.call("scde_hip_mode_fail_corr", mm, cd, bool(sq), modes, joint_posterior_modes(jp, g["prior_x"]))
    want = mode_relative_distance(models, cd, prior={"x": g["prior_x"]}, posteriors={"jp": jp, "modes": modes})
    assert np.array_equal((1 - got)[off], want[off], equal_nan=True)
    got = shim.call("scde_hip_direct_corr", mm, cd, bool(sq), 0.9, 3.0, None, 12345.0)
    want = direct_dropout_distance(models, cd, n_simulations=3, k=0.9, seed=12345)
    assert np.array_equal((1 - got)[off], want[off], equal_nan=True)
    unif = np.random.default_rng(2).random((2, 20, 50))
    got = shim.call("scde_hip_direct_corr", mm, cd, bool(sq), 0.9, 2, unif.ravel(), 0.0)
    want = direct_dropout_distance(models, cd, n_simulations=2, k=0.9, uniforms=unif)
    assert np.array_equal((1 - got)[off], want[off], equal_nan=True)
