"""The mixture cross-fit of cell pairs on the GPU (scde_amd/error_models.py crossfit_models and
crossfit=; csrc/crossfit_fit.hip, csrc/error_models.hip) against the numpy restatement of its
contract (tests/crossfit_ref.py).  No result here can be compared with a
run of R: the data files ship no stored threshold.segmentation = FALSE result.

The pair fit is held to the bounds tests/test_gpu_error_models.py holds nb2_fit_models to (the
same solvers): per quantity, 100 x the restatement's own spread over three gene permutations, at
least 1e-10; coefficients relative to max(1, |.|), theta and llh relative, posteriors absolute.
The reduction of the threshold rule's clusters is tied to scde_crossfit_inputs_*, which is
checked against R's stored models.
"""
import itertools

import numpy as np
import pytest

import crossfit_cases as K
import crossfit_ref as R
import error_models_ref as E
from conftest import golden

pytestmark = pytest.mark.gpu

FLOOR = 1e-10


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def param_spread(r, q):
    d = np.abs(q - r) / np.maximum(1.0, np.abs(r))
    d[[6, 9]] = np.abs(q[[6, 9]] - r[[6, 9]]) / np.abs(r[[6, 9]])
    return d


def permutation_spread(c1, c2, fit, n=3):
    """The restatement's own spread over gene permutations: (params (10), llh, posterior); None
    when a permutation changes the status or the number of rounds."""
    sp, sl, spo = np.zeros(10), 0.0, 0.0
    for s in range(1, n + 1):
        o = np.random.default_rng(s).permutation(len(c1))
        p = R.fit_pair(c1[o], c2[o])
        if p["status"] != fit["status"] or p["iterations"] != fit["iterations"]:
            return None
        if fit["status"] != 0:
            continue
        sp = np.maximum(sp, param_spread(fit["params"], p["params"]))
        sl = max(sl, abs(p["llh"] - fit["llh"]) / abs(fit["llh"]))
        back = np.empty_like(p["posterior"])
        back[o] = p["posterior"]
        rows = fit["rows"]
        spo = max(spo, float(np.max(np.abs(back[rows] - fit["posterior"][rows]))))
    return sp, sl, spo


def compare_pair(got, p, fit, spread, what):
    """One pair of a crossfit_models result against its restatement at the module's bounds."""
    assert got["status"][p] == fit["status"], (what, got["status"][p], fit["status"])
    assert got["iterations"][p] == fit["iterations"], (what, got["iterations"][p], fit["iterations"])
    cl, po = got["clusters"][:, p], got["posterior"][:, :, p]
    if fit["status"] != 0:
        assert np.all(np.isnan(got["params"][p])) and np.isnan(got["llh"][p]), what
        assert np.all(cl == 0) and np.all(np.isnan(po)), what
        return
    sp, sl, spo = spread
    dq = param_spread(fit["params"], got["params"][p])
    dl = abs(got["llh"][p] - fit["llh"]) / abs(fit["llh"])
    rows = fit["rows"]
    out = np.setdiff1d(np.arange(len(cl)), rows)
    assert np.all(cl[out] == 0) and np.all(np.isnan(po[:, out])), what
    dp = float(np.max(np.abs(po[:, rows].T - fit["posterior"][rows][:, [0, 2]])))
    print(f"{what}: params {dq.max():.3g} (bound {max(FLOOR, 100 * sp.max()):.3g}), llh {dl:.3g}, posterior {dp:.3g}")
    assert np.all(dq <= np.maximum(FLOOR, 100 * sp)), (what, dq, sp)
    assert dl <= max(FLOOR, 100 * sl), (what, dl, sl)
    tol = max(FLOOR, 100 * spo)
    assert dp <= tol, (what, dp, spo)
    top = np.sort(fit["posterior"][rows], axis=1)
    clear = top[:, 2] - top[:, 1] > tol
    np.testing.assert_array_equal(cl[rows][clear], fit["clusters"][rows][clear], err_msg=what)
    assert np.all((cl[rows] >= 1) & (cl[rows] <= 3)), what


# ------------------------------------------------------------------ shared inputs and references
@pytest.fixture(scope="module")
def esmef():
    """The 6 + 5 cells of the ES/MEF fixture, their 25 pairs and the restatement's fits."""
    from scde_amd import error_models as EM
    g = golden("esmef500.npz")
    cells = list(K.ES_CELLS + K.MEF_CELLS)
    counts = np.asfortranarray(g["counts"][:, cells])
    groups = np.array([0] * 6 + [1] * 5)
    pairs = EM.crossfit_pairs(groups)
    assert pairs.shape == (2, 25)
    ref = R.crossfit(counts, pairs)
    assert np.all(ref["status"] == 0), ref["status"]  # (the restatement fits all 25 pairs)
    return counts, groups, pairs, ref


@pytest.fixture(scope="module")
def shapes():
    """500 genes x 20 cells, ten pairs: 1, 63, 64, 65, 255, 256 and 257 rows (trailing all-zero
    genes), a pair with no rows, two identical high-count cells (component lost) and the
    fixture's cells 1 and 13 (a separable concomitant: status 3 in the first round)."""
    g = golden("esmef500.npz")
    N = 500
    counts = np.zeros((N, 20), np.int32, order="F")
    for k, n in enumerate(K.ROWS):
        counts[:, 2 * k:2 * k + 2] = K.synthetic_pair(n, 100 * n, N)
    counts[:40, 16] = counts[:40, 17] = np.arange(50, 90)
    counts[:, 18], counts[:, 19] = g["counts"][:, 1], g["counts"][:, 13]
    pairs = np.array([np.arange(0, 20, 2), np.arange(1, 20, 2)], np.int32)
    groups = np.repeat(np.arange(10), 2)
    fits = [R.fit_pair(counts[:, i], counts[:, j]) for i, j in pairs.T]
    assert [len(f["rows"]) for f in fits[:8]] == list(K.ROWS) + [0]
    assert [f["status"] for f in fits] == [6, 0, 0, 0, 0, 0, 0, 1, 6, 3]
    x = (np.log(counts[fits[9]["rows"], 18] + 1.0) + np.log(counts[fits[9]["rows"], 19] + 1.0)) / 2
    y1, y2 = counts[fits[9]["rows"], 18], counts[fits[9]["rows"], 19]
    start = np.stack([y1 <= 4, (y1 > 4) & (y2 > 4), y2 <= 4]).astype(float)
    assert np.all(np.isnan(R.concomitant3(x, start / start.sum(axis=0))))  # (status 3 is the concomitant's)
    return counts, groups, pairs, fits


@pytest.fixture(scope="module")
def shapes_run(shapes):
    from scde_amd import error_models as EM
    counts, groups, pairs, _ = shapes
    return EM.crossfit_models(counts, groups, pairs=pairs)


def same_bits(a, b, keys=("status", "iterations", "llh", "params", "clusters", "posterior")):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if x.dtype.kind == "f":
            np.testing.assert_array_equal(bits(x), bits(y), err_msg=k)
        else:
            np.testing.assert_array_equal(x, y, err_msg=k)


# ------------------------------------------------------------------ 1. the anchor
def test_threshold_rule_through_the_reduction_is_error_model_inputs():
    from scde_amd import error_models as EM
    g = golden("esmef500.npz")
    cells = list(range(6)) + list(range(20, 26))
    counts = np.asfortranarray(g["counts"][:, cells])
    groups = np.array([0] * 6 + [1] * 6)
    want = EM.error_model_inputs(counts, groups, min_size_entries=200)
    cf = R.threshold_crossfit(counts, want["pairs"], 4)
    assert set(np.unique(cf["clusters"])) == {0, 1, 2, 3}
    got = EM.error_model_inputs(counts, groups, min_size_entries=200, crossfit=cf)
    np.testing.assert_array_equal(got["ls"], want["ls"])
    np.testing.assert_array_equal(got["nabove"], want["nabove"])
    np.testing.assert_array_equal(got["vi"], want["vi"])
    assert 0 < want["vi"].sum() < want["vi"].size
    np.testing.assert_array_equal(got["vil"] != 0, counts >= 4)
    np.testing.assert_array_equal(bits(got["fpm"]), bits(want["fpm"]))
    v = want["vi"]
    print("fail_prior: largest relative difference %.3g" % np.max(np.abs(got["fail_prior"][v] / want["fail_prior"][v] - 1)))
    np.testing.assert_allclose(got["fail_prior"][v], want["fail_prior"][v], rtol=1e-13, atol=0)
    assert np.all(np.isnan(got["fail_prior"][~v]))


# ------------------------------------------------------------------ 2. the pair fit
def test_pair_fit_against_the_restatement(esmef):
    from scde_amd import error_models as EM
    counts, groups, pairs, ref = esmef
    got = EM.crossfit_models(counts, groups)
    np.testing.assert_array_equal(got["pairs"], pairs)
    assert got["clusters"].shape == (500, 25) and got["clusters"].dtype == np.int8
    assert got["posterior"].shape == (2, 500, 25) and got["params"].shape == (25, 10)
    for p, (i, j) in enumerate(pairs.T):
        fit = ref["fits"][p]
        spread = permutation_spread(counts[:, i], counts[:, j], fit)
        assert spread is not None, f"pair {p}: the restatement is not stable under gene permutations"
        compare_pair(got, p, fit, spread, f"pair {p} ({i}, {j})")


# ------------------------------------------------------------------ 3. shapes where the kernel can go wrong
def test_row_counts_and_failure_statuses(shapes, shapes_run):
    counts, _, pairs, fits = shapes
    for p, (i, j) in enumerate(pairs.T):
        spread = permutation_spread(counts[:, i], counts[:, j], fits[p])
        assert spread is not None, p
        compare_pair(shapes_run, p, fits[p], spread, f"pair {p}: {len(fits[p]['rows'])} rows")


def test_lds_rows_forced_to_one_gives_the_same_bits(shapes, shapes_run):
    from scde_amd import error_models as EM
    counts, groups, pairs, _ = shapes
    same_bits(EM.crossfit_models(counts, groups, pairs=pairs, lds_rows=1), shapes_run)


def test_a_pair_alone_two_runs_and_both_entries_give_the_same_bits(shapes, shapes_run):
    from scde_amd import api, error_models as EM
    counts, groups, pairs, _ = shapes
    same_bits(EM.crossfit_models(counts, groups, pairs=pairs), shapes_run)
    for p in (3, 6, 9):
        one = EM.crossfit_models(counts, groups, pairs=pairs[:, p:p + 1])
        same_bits(one, {k: (v[..., p:p + 1] if k in ("clusters", "posterior") else v[p:p + 1])
                        for k, v in shapes_run.items() if k not in ("pairs", "min_count_threshold")})
    dc = api.DeviceCounts(api.default_context(), counts)
    try:
        same_bits(EM.crossfit_models(dc, groups, pairs=pairs), shapes_run)
    finally:
        dc.free()


def test_null_outputs_are_accepted(shapes, shapes_run):
    """Every output NULL: the fit still runs and leaves its results resident for the reduction."""
    from scde_amd import api
    from scde_amd._lib import check, lib
    counts, groups, pairs, _ = shapes
    keep = np.flatnonzero(shapes_run["status"] == 0)
    pr = np.ascontiguousarray(pairs[:, keep])
    cells = np.unique(pr)
    sub = np.asfortranarray(counts[:, cells])
    pr = np.ascontiguousarray(np.searchsorted(cells, pr).astype(np.int32))
    N, C, P = sub.shape[0], sub.shape[1], pr.shape[1]
    codes = np.ascontiguousarray(np.repeat(np.arange(C // 2), 2).astype(np.int32))
    check(lib().scde_crossfit_fit_host(None, api._p(sub), N, N, C, api._p(pr), P, 4, 1e-5, 0.1, 200, 0, None, None,
                                       None, None, None, None))
    vil = np.zeros((N, C), np.uint8, order="F")
    check(lib().scde_crossfit_reduce_host(None, api._p(sub), N, N, C, api._p(codes), None, api._p(pr), P, None, None,
                                          None, 3, api._p(vil), None, None, None))
    full = {"pairs": pr, "status": np.zeros(P, np.int32), "clusters": shapes_run["clusters"][:, keep],
            "posterior": shapes_run["posterior"][:, :, keep]}
    want = R.reduce(sub, codes, full, np.ones(C), 3)["vil"]
    np.testing.assert_array_equal(vil != 0, want)
    assert want.any() and not want.all()


def test_more_pairs_than_compute_units():
    from scde_amd import error_models as EM
    counts = K.many_cells()
    got = EM.crossfit_models(counts)
    pl = list(itertools.combinations(range(26), 2))
    assert got["pairs"].shape == (2, 325) and [tuple(p) for p in got["pairs"].T] == pl
    seen = set()
    for p in (0, 1, 255, 256, 257, 300, 324):
        i, j = pl[p]
        fit = R.fit_pair(counts[:, i], counts[:, j])
        spread = permutation_spread(counts[:, i], counts[:, j], fit)
        assert spread is not None, p
        compare_pair(got, p, fit, spread, f"pair {p} of 325")
        seen.add(fit["status"])
    assert seen == {0, 3}
    half = EM.crossfit_models(counts, pairs=got["pairs"][:, 163:])
    same_bits(half, {k: (v[..., 163:] if k in ("clusters", "posterior") else v[163:])
                     for k, v in got.items() if k not in ("pairs", "min_count_threshold")})


# ------------------------------------------------------------------ 4. counts to models
def test_error_models_with_the_mixture_crossfit(esmef):
    from scde_amd import error_models as EM, knn
    counts, groups, pairs, ref = esmef
    jmm, det = EM.scde_error_models(counts, groups, crossfit="mixture", linear_fit=False, min_size_entries=200,
                                    return_details=True)
    assert np.all(det["status"] == 0) and jmm.shape == (11, 6)
    same = det["crossfit"]
    np.testing.assert_array_equal(same["status"], ref["status"])
    np.testing.assert_array_equal(same["iterations"], ref["iterations"])
    # the restatement, chained: its pair fits, R's library sizes from its vil, its reduction, its nb2 fit
    vil = R.reduce(counts, groups, ref, np.ones(11), 3)["vil"]
    ls = knn.estimate_library_sizes(counts, 200, 4, vil=vil)
    np.testing.assert_array_equal(det["inputs"]["vil"] != 0, vil)
    np.testing.assert_array_equal(det["inputs"]["ls"], ls)
    want = R.reduce(counts, groups, ref, ls, 3)
    np.testing.assert_array_equal(det["inputs"]["vi"], want["vi"])
    np.testing.assert_array_equal(det["inputs"]["nabove"], want["nabove"])
    v = want["vi"]
    np.testing.assert_allclose(det["inputs"]["fpm"][v], want["fpm"][v], rtol=1e-14)
    # (a chained comparison, at the bound the existing chained nb2 check uses for the models)
    np.testing.assert_allclose(det["inputs"]["fail_prior"][v], want["fail_prior"][v], rtol=1e-8)
    for c in range(11):
        fit = E.fit_cell_nb2(counts[v[:, c], c], want["fpm"][v[:, c], c], want["fail_prior"][v[:, c], c])
        assert fit["status"] == 0 and det["iterations"][c] == fit["iterations"], c
        np.testing.assert_allclose(jmm.to_numpy()[c], fit["row"][:6], rtol=1e-8, err_msg=str(c))
    # the same call in three steps, bit for bit
    cf = EM.crossfit_models(counts, groups)
    same_bits(cf, same)
    inputs = EM.error_model_inputs(counts, groups, min_size_entries=200, crossfit=cf)
    for k in ("fpm", "fail_prior"):
        np.testing.assert_array_equal(bits(inputs[k]), bits(det["inputs"][k]), err_msg=k)
    mm = EM.nb2_fit_models(inputs, counts)
    np.testing.assert_array_equal(bits(mm[:, :6]), bits(jmm.to_numpy()))
    again = EM.error_model_inputs(counts, groups, min_size_entries=200, crossfit="mixture")
    for k in ("fpm", "fail_prior", "ls"):
        np.testing.assert_array_equal(bits(again[k]), bits(inputs[k]), err_msg=k)


def test_failed_pairs_warn_and_drop(esmef):
    """The six ES cells and a copy of the first as one group: the pair of identical cells fails
    (a separable concomitant) and is dropped; as a cell's only pair it is an error."""
    from scde_amd import error_models as EM
    counts = esmef[0]
    sub = np.asfortranarray(np.column_stack([counts[:, :6], counts[:, 0]]))  # cell 6 repeats cell 0
    pairs = np.array([[0, 0, 0, 1, 2, 3, 4, 0], [1, 2, 3, 2, 3, 4, 5, 6]], np.int32)
    with pytest.warns(UserWarning, match="cross-fit of cells 0 and 6 failed"), pytest.raises(ValueError,
                                                                                            match="cell 6 failed"):
        EM.error_model_inputs(sub, pairs=pairs, min_size_entries=100, crossfit="mixture")
    pairs = np.column_stack([pairs, [[5], [6]]]).astype(np.int32)
    with pytest.warns(UserWarning, match="cross-fit of cells 0 and 6 failed"):
        got = EM.error_model_inputs(sub, pairs=pairs, min_size_entries=100, min_nonfailed=2, crossfit="mixture")
    cf = got["crossfit"]
    assert cf["status"][7] == 3 and np.all(np.delete(cf["status"], 7) == 0)
    full = EM.crossfit_models(sub, pairs=pairs)
    want = R.reduce(sub, np.zeros(7, int), full, got["ls"], 2)
    np.testing.assert_array_equal(got["vi"], want["vi"])
    np.testing.assert_array_equal(got["nabove"], want["nabove"])
    np.testing.assert_allclose(got["fail_prior"][want["vi"]], want["fail_prior"][want["vi"]], rtol=1e-13)


# ------------------------------------------------------------------ 5. fits against a reference
def test_fit_models_to_reference():
    import pandas as pd
    from scde_amd import error_models as EM
    g = golden("esmef500.npz")
    counts = g["counts"][:, :8]
    names = [str(c) for c in g["cells"][:8]]
    ref = g["counts"].sum(axis=1)
    f = ref / ref.sum() * 1e6
    for min_fpm in (1, 700):
        use = f > min_fpm
        assert (min_fpm == 1) == bool(use.all()) and use.sum() > 100
        jmm = EM.scde_fit_models_to_reference(pd.DataFrame(counts, columns=names), ref, min_fpm=min_fpm)
        assert list(jmm.index) == names and list(jmm.columns) == ["conc.b", "conc.a", "fail.r", "corr.b", "corr.a",
                                                                  "corr.theta"]
        for c in range(8 if min_fpm == 1 else 2):
            y = counts[use, c]
            fit = E.fit_cell_nb2(y, f[use], np.where(y <= 1, 1.0, 0.0))
            assert fit["status"] == 0
            d = E.row_spread(fit["row"], jmm.to_numpy()[c])
            print(f"cell {c}, min_fpm {min_fpm}: {max(d.values()):.3g}")
            assert max(d.values()) <= 1e-8, (c, d)
    with pytest.raises(RuntimeError, match="building a model for cell"):
        EM.scde_fit_models_to_reference(np.zeros((500, 2), np.int32), ref)
