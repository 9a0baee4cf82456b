"""knn.error.models' mixture fit on the GPU (scde_amd/knn.py knn_fit_models / knn_error_models,
csrc/knn_fit.hip) against the numpy restatement of its contract (tests/knn_fit_ref.py, DESIGN.md
section 4.15) and against R's stored models of the pollen data.

What is compared how tightly follows what was measured on the restatement itself, rerun on gene
permutations (a rounding-level perturbation): one M-step and the constant-theta EM are stable to
rounding and are compared tightly; the chained local-theta EM is not for every cell, so each
cell's tolerance is taken from the restatement's own spread (knn_fit_ref.reference).
The cells come from knn_fit_ref.synthetic_cell; the seeds of the lists below were chosen by
scanning the generator for cells on which the restatement alone is stable, and for cells with a
curve parameter on its bound.
"""
import math
import warnings

import numpy as np
import pytest

import knn_fit_ref as F
from conftest import GOLD, golden

pytestmark = pytest.mark.gpu

NS = [3, 5, 63, 64, 65, 257, 1025]
ONE_STEP_SEED = {3: 103, 5: 105, 63: 213, 64: 414, 65: 215, 257: 457, 1025: 1225}
EPS = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def pack(cells, pad=9, seed=0):
    """genes x cells inputs holding each cell's valid genes at sorted random rows; the other
    entries hold counts and magnitudes the fit must not read (fail prior NaN)."""
    rng = np.random.default_rng(seed)
    N = max(len(c[0]) for c in cells) + pad
    C = len(cells)
    counts = rng.integers(0, 50, (N, C)).astype(np.int32)
    fpm = rng.random((N, C)) * 10
    fp = np.full((N, C), np.nan)
    rows = []
    for j, (y, x, f) in enumerate(cells):
        r = np.sort(rng.choice(N, len(y), replace=False))
        counts[r, j], fpm[r, j], fp[r, j] = y, x, f
        rows.append(r)
    return np.asfortranarray(counts), {"fpm": np.asfortranarray(fpm), "fail_prior": np.asfortranarray(fp)}, rows


def run(cells, dev=False, **kw):
    from scde_amd import api, knn
    counts, inputs, rows = pack(cells)
    if dev:
        dc = api.DeviceCounts(api.default_context(), counts)
        try:
            mm, det = knn.knn_fit_models(inputs, dc, return_details=True, **kw)
        finally:
            dc.free()
    else:
        mm, det = knn.knn_fit_models(inputs, counts, return_details=True, **kw)
    det["rows"] = rows
    return mm, det


def start_weights(cell, a, theta_range=(1e-2, 1e2)):
    y, x, fp = cell
    al = F.alpha_of(y.astype(np.float64), a * x, theta_range)
    return np.log(x), np.log(al), (1 - fp) * np.sqrt(al)


def check_one_step(mm, det, j, ref, what):
    cell, fit = ref["cell"], ref["fit"]
    assert det["status"][j] == fit["status"] == 0, what
    assert det["iterations"][j] == 1
    row, want = mm[j], fit["row"]
    fig = {"a": abs(math.expm1(row[3] - want[3])), "llh": abs(det["llh"][j] - fit["llh"]) / abs(fit["llh"]),
           "theta": abs(row[5] - want[5]) / want[5],
           "beta": max(abs(row[c] - want[c]) / max(1.0, abs(want[c])) for c in (0, 1, 11))}
    grid = F.curve_grid(cell[1])
    fig["curve"] = float(np.max(np.abs(F.curve(row[6:11], grid) - F.curve(want[6:11], grid))))
    l, la, W = start_weights(cell, math.exp(want[3]))
    og, ow = F.curve_objective(row[6:11], l, la, W), F.curve_objective(want[6:11], l, la, W)
    # below this the objective is its own evaluation's rounding: a residual la - f carries about
    # 4 eps |la|, so the sum cannot be resolved under 16 eps^2 sum W la^2 (an exact fit of 3 or 5 genes)
    floor = 16 * EPS * EPS * float(np.sum(W * la * la))
    tol_curve = max(1e-10, 100 * ref["curve_spread"])
    print(what, {k: f"{v:.2e}" for k, v in fig.items()}, f"objective {og:.6e} vs {ow:.6e}",
          f"curve tolerance {tol_curve:.1e}")
    assert fig["a"] <= 1e-12 and fig["llh"] <= 1e-12, what
    assert fig["theta"] <= 1e-10, what
    assert fig["beta"] <= 1e-8, what
    assert fig["curve"] <= tol_curve, what
    assert og <= ow * (1 + 1e-9) + floor, what
    assert np.all(row[6:11] >= F.BOX_LO) and np.all(row[6:11] <= F.BOX_HI)
    assert row[2] == math.log(0.1) and row[4] == 1.0
    p1 = det["posteriors"][det["rows"][j], j]
    np.testing.assert_allclose(p1, fit["p1"], rtol=0, atol=max(1e-9, 100 * ref["spread"]))
    away = np.abs(fit["p1"] - 0.5) > 1e-6
    np.testing.assert_array_equal(det["clusters"][det["rows"][j], j][away], fit["clusters"][away])


# ------------------------------------------------------------------ one step
@pytest.mark.parametrize("n", NS)
def test_one_step_one_cell(n):
    ref = F.reference(n, ONE_STEP_SEED[n], iter=1, permutations=3)
    mm, det = run([ref["cell"]], iter=1)
    check_one_step(mm, det, 0, ref, f"n = {n}")
    outside = np.setdiff1d(np.arange(det["clusters"].shape[0]), det["rows"][0])
    assert np.all(det["clusters"][outside, 0] == 0) and np.all(np.isnan(det["posteriors"][outside, 0]))


def test_one_step_three_cells_of_different_size():
    refs = [F.reference(n, ONE_STEP_SEED[n], iter=1, permutations=3) for n in (1025, 63, 257)]
    mm, det = run([r["cell"] for r in refs], iter=1)
    for j, r in enumerate(refs):
        check_one_step(mm, det, j, r, f"cell {j} of 3")


def test_one_step_600_cells_of_40_genes():
    """More cells than workgroups are resident: the groups stride over the cells."""
    cells = [F.synthetic_cell(40, 3000 + j) for j in range(600)]
    mm, det = run(cells, iter=1)
    assert np.all(det["iterations"][det["status"] == 0] == 1)
    assert np.all(np.isfinite(mm[det["status"] == 0][:, :12]))
    assert np.all(np.isnan(mm[det["status"] != 0]))
    # every 23rd cell on which the restatement itself is stable to rounding (its own spread over
    # gene permutations at most 1e-13: a 40-gene curve fit often is not, and then an llh cannot be
    # compared to 1e-12); the choice looks at the restatement alone
    checked = 0
    for j in range(7, 600, 23):
        ref = F.reference(40, 3000 + j, iter=1, permutations=3)
        if ref["fit"]["status"] != 0:
            assert det["status"][j] == ref["fit"]["status"]
            continue
        if ref["spread"] > 1e-13:
            continue
        check_one_step(mm, det, j, ref, f"cell {j} of 600")
        checked += 1
    assert checked >= 8
    for j in (0, 255, 256, 599):
        alone, _ = run([cells[j]], iter=1)
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))


# ------------------------------------------------------------------ whole EM
def test_constant_theta_em():
    refs = [F.reference(n, ONE_STEP_SEED[n], local_theta=False) for n in NS]
    mm, det = run([r["cell"] for r in refs], local_theta_fit=False)
    for j, (n, r) in enumerate(zip(NS, refs)):
        fit = r["fit"]
        assert det["status"][j] == fit["status"], n
        if fit["status"] != 0:
            continue
        cols = [0, 1, 3, 5, 11]
        rel = np.abs(mm[j, cols] - fit["row"][cols]) / np.abs(fit["row"][cols])
        print(f"n = {n}: iterations {det['iterations'][j]} / {fit['iterations']}, relative differences", rel)
        assert np.all(rel <= 1e-9), n
        assert np.all(np.isnan(mm[j, 6:11]))
        assert det["iterations"][j] == fit["iterations"], n
        assert abs(det["llh"][j] - fit["llh"]) <= 1e-9 * abs(fit["llh"])
        away = np.abs(fit["p1"] - 0.5) > 1e-6
        np.testing.assert_array_equal(det["clusters"][det["rows"][j], j][away], fit["clusters"][away])


LOCAL_SEEDS = [0, 1, 2, 3, 4, 5, 8, 10, 11]  # 250 genes each; seed 0 is the ill-conditioned one


@pytest.fixture(scope="module")
def local_em():
    cells = [F.synthetic_cell(250, s) for s in LOCAL_SEEDS]
    return run(cells)


@pytest.mark.parametrize("j", range(len(LOCAL_SEEDS)))
def test_local_theta_em(local_em, j):
    mm, det = local_em
    ref = F.reference(250, LOCAL_SEEDS[j], permutations=3)
    fit = ref["fit"]
    assert det["status"][j] == fit["status"] == 0
    dl = abs(det["llh"][j] - fit["llh"])
    if ref["curve_spread"] > 1e-5:
        print(f"seed {LOCAL_SEEDS[j]}: ill-conditioned (curve spread {ref['curve_spread']:.2e}); llh differs by "
              f"{dl:.2e}, the restatement's own spread is {ref['llh_spread']:.2e}")
        assert dl <= 10 * ref["llh_spread"]
        return
    tol = max(1e-8, 100 * ref["spread"])
    row, want = mm[j], fit["row"]
    grid = F.curve_grid(ref["cell"][1])
    fig = {"corr.b": abs(row[3] - want[3]), "theta": abs(row[5] - want[5]) / want[5],
           "beta": max(abs(row[c] - want[c]) / max(1.0, abs(want[c])) for c in (0, 1, 11)),
           "curve": float(np.max(np.abs(F.curve(row[6:11], grid) - F.curve(want[6:11], grid)))),
           "llh": dl / abs(fit["llh"])}
    print(f"seed {LOCAL_SEEDS[j]}: tolerance {tol:.1e}", {k: f"{v:.2e}" for k, v in fig.items()},
          f"iterations {det['iterations'][j]} / {fit['iterations']}")
    for k, v in fig.items():
        assert v <= tol, k


def test_local_theta_list_is_mostly_well_conditioned():
    """(after the cases above: the restatement's fits are shared with them)"""
    ill = [s for s in LOCAL_SEEDS if F.reference(250, s, permutations=3)["curve_spread"] > 1e-5]
    assert len(LOCAL_SEEDS) >= 8 and len(ill) <= len(LOCAL_SEEDS) // 4, ill


# ------------------------------------------------------------------ the same bits
def test_entries_repeat_and_agree_bit_for_bit():
    cells = [F.synthetic_cell(n, 40 + n) for n in (65, 257, 1025, 5)]
    mm, det = run(cells)
    again, det2 = run(cells)
    dev, det3 = run(cells, dev=True)
    for other, d in ((again, det2), (dev, det3)):
        np.testing.assert_array_equal(bits(other), bits(mm))
        np.testing.assert_array_equal(bits(d["llh"]), bits(det["llh"]))
        np.testing.assert_array_equal(bits(d["posteriors"]), bits(det["posteriors"]))
        np.testing.assert_array_equal(d["clusters"], det["clusters"])
        np.testing.assert_array_equal(d["iterations"], det["iterations"])
    for j in (0, 2):
        alone, da = run([cells[j]])
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))
        assert da["iterations"][0] == det["iterations"][j]
        np.testing.assert_array_equal(bits(da["posteriors"][da["rows"][0], 0]),
                                      bits(det["posteriors"][det["rows"][j], j]))


@pytest.mark.parametrize("lds_genes", [100, 3])
def test_cells_too_large_for_lds_give_the_same_bits(lds_genes):
    """With lds_genes below a cell's valid genes its vectors live in the HBM workspace."""
    cells = [F.synthetic_cell(n, 40 + n) for n in (63, 257, 1025)]
    mm, det = run(cells, iter=3)
    ws, dws = run(cells, iter=3, lds_genes=lds_genes)
    np.testing.assert_array_equal(bits(ws), bits(mm))
    np.testing.assert_array_equal(bits(dws["posteriors"]), bits(det["posteriors"]))


# ------------------------------------------------------------------ edges
def test_theta_on_its_bounds():
    po = F.reference(257, 7, local_theta=False, drop=False, theta_kind="poisson")
    # a million reads on the three genes of smallest magnitude, none elsewhere: the deviance is
    # above its expectation at every theta of the range
    rng = np.random.default_rng(5)
    x = np.exp(rng.normal(2, 1.6, 400))
    y = np.zeros(400, np.int32)
    y[np.argsort(x)[:3]] = 1000000
    fp = np.where(y <= 1, 0.3, 1e-6)
    with np.errstate(all="ignore"):
        wild = F.fit_cell(y, x, fp, local_theta=False, iter=1)
    assert po["fit"]["row"][5] == 100.0 and wild["row"][5] == 0.01  # the restatement is on the bounds
    mm, det = run([po["cell"]], local_theta_fit=False)
    assert mm[0, 5] == 100.0 and det["iterations"][0] == po["fit"]["iterations"]
    assert abs(mm[0, 3] - po["fit"]["row"][3]) <= 1e-9
    mm, det = run([(y, x, fp)], local_theta_fit=False, iter=1)
    assert det["status"][0] == 0 and mm[0, 5] == 0.01
    assert abs(det["llh"][0] - wild["llh"]) <= 1e-12 * abs(wild["llh"])


@pytest.mark.parametrize("n,seed", [(1025, 1125), (65, 165), (65, 265)])
def test_curve_parameter_on_its_bound(n, seed):
    ref = F.reference(n, seed, iter=1, permutations=3)
    want = ref["fit"]["row"][6:11]
    on = (want == F.BOX_LO) | (want == F.BOX_HI)
    assert on.any()
    mm, det = run([ref["cell"]], iter=1)
    np.testing.assert_array_equal(mm[0, 6:11][on], want[on])
    check_one_step(mm, det, 0, ref, f"n = {n}, seed {seed}")


def test_failed_cells_leave_the_others_alone():
    good = [F.synthetic_cell(65, 11), F.synthetic_cell(257, 12)]
    y, x, fp = F.synthetic_cell(40, 13)
    zeros = (np.zeros(40, np.int32), x, fp)
    tiny = (y[:2], x[:2], fp[:2])
    none = (y[:0], x[:0], fp[:0])
    mm, det = run([good[0], zeros, tiny, good[1], none], iter=4)
    np.testing.assert_array_equal(det["status"], [0, 3, 1, 0, 1])
    for j in (1, 2, 4):
        assert np.all(np.isnan(mm[j])) and np.isnan(det["llh"][j])
        assert np.all(det["clusters"][:, j] == 0) and np.all(np.isnan(det["posteriors"][:, j]))
    for j, c in ((0, good[0]), (3, good[1])):
        alone, _ = run([c], iter=4)
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))


def small_counts(N=400, C=14, seed=2):
    rng = np.random.default_rng(seed)
    lam = rng.gamma(0.7, 30.0, size=(N, 1)) * rng.uniform(0.5, 2.0, size=(1, C))
    counts = rng.poisson(lam * rng.gamma(2.0, 0.5, size=(N, C))) * (rng.random((N, C)) < 0.7)
    return np.asfortranarray(counts.astype(np.int32))


def test_error_models_drops_a_failed_cell_with_a_warning():
    from scde_amd import knn
    from scde_amd.models import MODEL_COLUMNS
    counts = small_counts()
    counts[:, 5] = 0  # a cell without a read: its slope is 0 and its fit fails
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        jmm, det = knn.knn_error_models(counts, k=5, min_nonfailed=2, min_size_entries=200, return_details=True)
    assert det["status"][5] != 0 and np.all(np.delete(det["status"], 5) == 0)
    assert any("skipping the cell" in str(x.message) and "cell 5" in str(x.message) for x in w)
    assert list(jmm.columns) == MODEL_COLUMNS
    assert list(jmm.index) == [str(i) for i in range(14) if i != 5]
    assert np.all(np.isfinite(jmm.to_numpy()))
    # the fit alone, on the same inputs: the same bits
    mm = knn.knn_fit_models(det["inputs"], counts)
    np.testing.assert_array_equal(bits(jmm.to_numpy()), bits(np.delete(mm, 5, axis=0)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        flat = knn.knn_error_models(counts, k=5, min_nonfailed=2, min_size_entries=200, local_theta_fit=False)
    assert list(flat.columns) == [c for c in MODEL_COLUMNS if not c.startswith("corr.ltheta.")]


def test_error_models_with_groups_of_unequal_size():
    from scde_amd import knn
    counts = small_counts(seed=3)
    groups = np.array(["b"] * 5 + ["a"] * 9)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        jmm, det = knn.knn_error_models(counts, groups=groups, k=4, min_nonfailed=2, min_size_entries=200,
                                        return_details=True)
        mm = knn.knn_fit_models(det["inputs"], counts)
    assert np.all(det["status"] == 0)
    order = list(range(5, 14)) + list(range(5))  # R's rbind over the groups: "a" first
    assert list(jmm.index) == [str(i) for i in order]
    assert jmm.attrs["groups"] == ["a"] * 9 + ["b"] * 5
    np.testing.assert_array_equal(bits(jmm.to_numpy()), bits(mm[order]))
    nb = det["inputs"]["neighbours"]
    assert np.all(nb[:5][nb[:5] >= 0] < 5) and np.all(nb[5:][nb[5:] >= 0] >= 5)


def test_linear_fit_false_is_not_built():
    from scde_amd import knn
    counts = small_counts()
    with pytest.raises(NotImplementedError):
        knn.knn_error_models(counts, linear_fit=False)
    with pytest.raises(NotImplementedError):
        knn.knn_fit_models({}, counts, linear_fit=False)


def test_entry_errors():
    from scde_amd import _lib, knn
    counts, inputs, _ = pack([F.synthetic_cell(20, 1)])
    with pytest.raises(_lib.ScdeError, match="theta range"):
        knn.knn_fit_models(inputs, counts, theta_fit_range=(1.0, 1.0))
    with pytest.raises(_lib.ScdeError, match="max_iter"):
        knn.knn_fit_models(inputs, counts, iter=0)
    with pytest.raises(_lib.ScdeError, match="lds_genes"):
        knn.knn_fit_models(inputs, counts, lds_genes=100000)
    with pytest.raises(ValueError):
        knn.knn_fit_models({"fpm": inputs["fpm"][:5], "fail_prior": inputs["fail_prior"][:5]}, counts)


# ------------------------------------------------------------------ R's own result
# What the restatement measures against R's 64 stored rows (tests/test_knn_fit.py's module text;
# DESIGN.md section 4.15), last digit rounded up: median, 90th percentile, worst cell.  The GPU may
# differ from the restatement in another direction than R does: the bounds are 3 x these.
POLLEN_RESTATEMENT = {"corr.b": (5.88e-6, 7.27e-5, 0.0405), "theta": (4.23e-5, 5.72e-4, 0.0345),
                      "curve": (3.06e-4, 3.38e-3, 0.136), "conc": (2.32e-3, 1.10e-2, 0.115)}


def test_pollen_models_against_r():
    from scde_amd import knn, varnorm
    from scde_amd.models import MODEL_COLUMNS
    g = golden("pollen_knn.npz")
    counts = np.asfortranarray(g["counts"])
    jmm, det = knn.knn_error_models(counts, k=16, min_count_threshold=2, min_nonfailed=5, return_details=True)
    assert jmm.shape == (64, 12) and list(jmm.columns) == MODEL_COLUMNS
    got, ref = jmm.to_numpy(), g["models"]
    fpm, vi = det["inputs"]["fpm"], det["inputs"]["vi"]
    d = [F.row_distances(got[i], ref[i], np.log(fpm[vi[:, i], i])) for i in range(64)]
    print("iterations: median", np.median(det["iterations"]), "max", det["iterations"].max())
    for k, (med, p90, worst) in POLLEN_RESTATEMENT.items():
        v = np.array([x[k] for x in d])
        fig = (float(np.median(v)), float(np.quantile(v, 0.9)), float(v.max()))
        print(k, "median %.3g, 90th percentile %.3g, worst %.3g" % fig)
        assert fig[0] <= 3 * med and fig[1] <= 3 * p90 and fig[2] <= 3 * worst, k
    np.testing.assert_array_equal(got[:, 2], ref[:, 2])  # fail.r
    np.testing.assert_array_equal(got[:, 4], ref[:, 4])  # corr.a
    import os
    tab = varnorm.load_edf_table(os.path.join(GOLD, "scde_edff.npz"))
    vn = varnorm.pagoda_varnorm(jmm, counts, tab, n_randomizations=2, n_cores=1)
    assert vn["mat"].shape[1] == 64 and np.isfinite(vn["arv"]).any()
