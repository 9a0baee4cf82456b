"""The numpy restatement of R's ``dist`` (tests/rdist_ref.py) against scipy's ``pdist`` and on
hand-worked cases.  No GPU.

On NaN-free input the two differ only in the order of a p-term sum of non-negative terms, whose
relative error is at most p * 2^-52 to first order in either order (each of the at most p - 1
additions and the p products or absolute values rounds once, all terms of one sign); the square
root halves a relative error.  Equality is not asked for."""
import numpy as np
import pytest

import rdist_ref as R

SCIPY = {"euclidean": "euclidean", "manhattan": "cityblock", "maximum": "chebyshev"}


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("n,p", [(2, 1), (7, 3), (33, 65), (20, 700)])
def test_restatement_matches_pdist(method, n, p):
    from scipy.spatial.distance import pdist, squareform
    x = np.random.default_rng(n * 1000 + p).normal(size=(n, p)) * 10.0
    got = R.rdist(x, method)
    ref = squareform(pdist(x, SCIPY[method]))
    err = np.abs(got - ref)
    bound = p * 2.0 ** -52 * np.abs(ref)
    print(f"{method} {n} x {p}: max relative error {np.max(err / np.maximum(np.abs(ref), 1e-300)):.3g}, "
          f"bound {p * 2.0 ** -52:.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(got, got.T) and np.all(np.diag(got) == 0)


def test_hand_worked_nan_scaling():
    nan, inf = np.nan, np.inf
    x = np.array([[1.0, 2.0, nan, 4.0],
                  [2.0, nan, 1.0, 0.0],
                  [nan, nan, nan, nan],
                  [inf, 2.0, 3.0, 4.0],
                  [inf, 0.0, 3.0, 1.0]])
    e = R.rdist(x, "euclidean")
    # rows 0, 1 share columns 0 and 3: (1 + 16) / (2 / 4)
    assert e[1, 0] == np.sqrt(17.0 / 0.5)
    assert np.isnan(e[2, 0]) and np.isnan(e[2, 4]) and e[2, 2] == 0
    # rows 3, 4: Inf - Inf drops column 0; (4 + 0 + 9) / (3 / 4)
    assert e[4, 3] == np.sqrt(13.0 / 0.75)
    # rows 0, 3: Inf - 1 takes part
    assert e[3, 0] == inf
    m = R.rdist(x, "manhattan")
    assert m[1, 0] == 5.0 / 0.5 and m[4, 3] == 5.0 / 0.75
    c = R.rdist(x, "maximum")
    assert c[1, 0] == 4.0 and c[4, 3] == 3.0 and np.isnan(c[2, 1])


def test_sequential_order_is_what_is_summed():
    # 1 + 2^-53 + 2^-53 left to right stays 1; any other order gives 1 + 2^-52
    x = np.array([[1.0, 2.0 ** -53, 2.0 ** -53], [0.0, 0.0, 0.0]])
    assert R.rdist(x, "manhattan")[1, 0] == 1.0
    assert R.rdist(x[:, ::-1], "manhattan")[1, 0] == 1.0 + 2.0 ** -52


def test_unknown_method():
    with pytest.raises(ValueError):
        R.rdist(np.zeros((2, 2)), "minkowski")
