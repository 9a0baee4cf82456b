"""scde.error.models on the GPU (scde_amd/error_models.py; csrc/error_models.hip, csrc/nb2_fit.hip)
against the numpy restatements of its contract (tests/error_models_ref.py, DESIGN.md section
4.16) and against R's stored models of the ES/MEF data (``o.ifm``).

The input stage is compared with the *literal* restatement, which builds R's per-pair lists.  The
fit is compared with ``fit_cell_nb2`` at tolerances taken from the restatement alone: per
quantity, 100 x its own spread over three gene permutations (a rounding-level perturbation), at
least 1e-10.  The cells come from error_models_ref.synthetic_cell_nb2; their seeds were chosen by
scanning the generator on the CPU for cells on which the restatement is stable under gene
permutations and which take the branch wanted.  Spreads recorded there (largest over conc.b,
conc.a, corr.b, corr.a relative to max(1, |.|), and corr.theta relative):

    one round (iter = 1)                             full EM (iter = 50)
    3     sparse    24    2.5e-15                    2 rounds     5.1e-15
    5     negative  12    8.7e-16  negative slope    2 rounds     7.3e-16
    63    negative  63    2.5e-15  negative slope    fails in round 20 (status 3), every permutation
    64    underfit  106   4.8e-16  refit             25 rounds    3.2e-15  refit
    65    underfit  93    3.6e-15  refit             17 rounds    6.5e-15  refit
    65    large     72    8.3e-15  counts of 1e5     3 rounds     5.1e-15
    257   underfit  257   1.3e-15  refit             7 rounds     3.5e-15  refit
    257   negative  264   4.4e-16  negative slope    25 rounds    1.7e-15
    257   sparse    271   4.2e-14  254 genes y <= 1  19 rounds    3.5e-14
    1025  underfit  1025  2.2e-15  refit             8 rounds     4.4e-15  refit
    1025  large     1025  8.4e-15  counts of 1e5     3 rounds     9.2e-15
    1025  sparse    1046  2.6e-13  1022 genes y <= 1
    1025  plain     1025  7.3e-15                    9 rounds     3.0e-15

so every tolerance below is its floor, 1e-10, or close to it.  llh spreads are at most 8e-15
relative and the posteriors' at most 3e-15.
"""
import math
import warnings

import numpy as np
import pytest

import error_models_ref as E
from conftest import golden
from test_error_models import ESMEF_RESTATEMENT, distances_to_r

pytestmark = pytest.mark.gpu

ONE_ROUND = [(3, 24, "sparse"), (5, 12, "negative"), (63, 63, "negative"), (64, 106, "underfit"),
             (65, 93, "underfit"), (65, 72, "large"), (257, 257, "underfit"), (257, 264, "negative"),
             (257, 271, "sparse"), (1025, 1025, "underfit"), (1025, 1025, "large"), (1025, 1046, "sparse"),
             (1025, 1025, "plain")]
FULL_EM = [c for c in ONE_ROUND if c != (1025, 1046, "sparse")]
FLOOR = 1e-10


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
    from scde_amd import api, error_models as EM
    counts, inputs, rows = pack(cells)
    if dev:
        dc = api.DeviceCounts(api.default_context(), counts)
        try:
            mm, det = EM.nb2_fit_models(inputs, dc, return_details=True, **kw)
        finally:
            dc.free()
    else:
        mm, det = EM.nb2_fit_models(inputs, counts, return_details=True, **kw)
    det["rows"] = rows
    return mm, det


def check_fit(mm, det, j, ref, what):
    """Cell j of a launch against the restatement's fit, at the restatement's own tolerances."""
    fit = ref["fit"]
    assert ref["stable"], what  # (the list was chosen so)
    assert det["status"][j] == fit["status"], what
    assert det["iterations"][j] == fit["iterations"], what
    rows = det["rows"][j]
    if fit["status"] != 0:
        assert np.all(np.isnan(mm[j])) and np.isnan(det["llh"][j]), what
        assert np.all(det["clusters"][:, j] == 0) and np.all(np.isnan(det["posteriors"][:, j])), what
        return
    row, want = mm[j], fit["row"]
    fig = E.row_spread(want, row)
    tol = {c: max(FLOOR, 100 * ref["spread"][c]) for c in E.ROW_COLS}
    dl = abs(det["llh"][j] - fit["llh"]) / abs(fit["llh"])
    p1 = det["posteriors"][rows, j]
    dp = float(np.max(np.abs(p1 - fit["p1"])))
    print(what, {c: f"{v:.1e}/{tol[c]:.1e}" for c, v in fig.items()}, f"llh {dl:.1e} p1 {dp:.1e}",
          f"rounds {det['iterations'][j]}", "refit" if fit["refit"] else "",
          "negative slope" if fit["negative_slope"] else "")
    for c in E.ROW_COLS:
        assert fig[c] <= tol[c], (what, c)
    assert dl <= max(FLOOR, 100 * ref["llh_spread"]), what
    assert dp <= max(FLOOR, 100 * ref["p1_spread"]), what
    assert row[2] == math.log(0.1) and np.all(np.isnan(row[6:])), what
    away = np.abs(fit["p1"] - 0.5) > 1e-6
    np.testing.assert_array_equal(det["clusters"][rows, j][away], fit["clusters"][away])
    outside = np.setdiff1d(np.arange(det["clusters"].shape[0]), rows)
    assert np.all(det["clusters"][outside, j] == 0) and np.all(np.isnan(det["posteriors"][outside, j]))


# ------------------------------------------------------------------ 1. the inputs
def input_case(N):
    """Two groups of 2 and 5 cells, one of 3, one of 70 with sampled pairs; in the group of 5 a cell
    holding 1e6 reads beside cells holding 5 (a total minus the cell's own term would lose 16 bits)."""
    from scde_amd import error_models as EM
    codes = np.array([0, 0] + [1] * 5 + [2] * 3 + [3] * 70, np.int32)
    rng = np.random.default_rng(N)
    lam = rng.gamma(0.6, 12.0, size=(N, 1)) * rng.uniform(0.5, 2.0, size=(1, 80))
    counts = (rng.poisson(lam) * (rng.random((N, 80)) > 0.5)).astype(np.int32)
    counts[:, 2:7] = 5
    counts[:, 4] = 1000000
    order = rng.permutation(80)
    counts, codes = np.asfortranarray(counts[:, order]), codes[order]
    ls = rng.uniform(0.5, 2.0, 80)
    pairs = EM.crossfit_pairs(codes, max_pairs=40, min_pairs_per_cell=3, seed=1)
    return counts, codes, ls, pairs


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_inputs_against_the_literal_restatement(N):
    from scde_amd import api, error_models as EM
    counts, codes, ls, pairs = input_case(N)
    kw = dict(groups=codes, min_nonfailed=3, min_count_threshold=4, max_pairs=40, min_pairs_per_cell=3, seed=1,
              library_sizes=ls)
    got = EM.error_model_inputs(counts, **kw)
    np.testing.assert_array_equal(got["pairs"], pairs)
    ref = E.model_inputs(counts, codes, pairs, ls, 4, 3, literal=True)
    np.testing.assert_array_equal(got["vi"], ref["vi"])
    np.testing.assert_array_equal(got["nabove"], ref["nabove"])
    np.testing.assert_array_equal(np.isnan(got["fpm"]), np.isnan(ref["fpm"]))
    np.testing.assert_array_equal(np.isnan(got["fail_prior"]), np.isnan(ref["fail_prior"]))
    v = ref["vi"]
    ngroup = np.bincount(codes)[codes]
    rel = np.abs(got["fpm"] - ref["fpm"])[v] / ref["fpm"][v]
    assert np.all(rel <= (4 * ngroup * 2.0 ** -52)[None, :].repeat(N, 0)[v])
    np.testing.assert_allclose(got["fail_prior"][v], ref["fail_prior"][v], rtol=1e-13, atol=0)
    print(f"N = {N}: {int(v.sum())} valid entries, fpm off by at most {rel.max() if rel.size else 0:.1e}")
    # the same bits again, and from resident counts
    again = EM.error_model_inputs(counts, **kw)
    dc = api.DeviceCounts(api.default_context(), counts)
    try:
        dev = EM.error_model_inputs(dc, **kw)
    finally:
        dc.free()
    for other in (again, dev):
        for k in ("fpm", "fail_prior"):
            np.testing.assert_array_equal(bits(other[k]), bits(got[k]))
        np.testing.assert_array_equal(other["nabove"], got["nabove"])
    # a caller's pair list takes the place of the enumeration
    listed = EM.error_model_inputs(counts, pairs=pairs, groups=codes, library_sizes=ls)
    np.testing.assert_array_equal(bits(listed["fail_prior"]), bits(got["fail_prior"]))


def test_inputs_other_threshold_and_few_nonfailed():
    from scde_amd import error_models as EM
    counts, codes, ls, pairs = input_case(65)
    for thr, mnf in ((1, 1), (2, 6)):
        got = EM.error_model_inputs(counts, groups=codes, pairs=pairs, library_sizes=ls, min_count_threshold=thr,
                                    min_nonfailed=mnf)
        ref = E.model_inputs(counts, codes, pairs, ls, thr, mnf, literal=True)
        np.testing.assert_array_equal(got["vi"], ref["vi"])
        np.testing.assert_array_equal(got["nabove"], ref["nabove"])
        v = ref["vi"]
        np.testing.assert_allclose(got["fail_prior"][v], ref["fail_prior"][v], rtol=1e-13, atol=0)
        rel = np.abs(got["fpm"] - ref["fpm"])[v] / ref["fpm"][v]
        assert np.all(rel <= (4 * np.bincount(codes)[codes] * 2.0 ** -52)[None, :].repeat(65, 0)[v])


def test_input_entry_errors():
    from scde_amd import _lib, api, error_models as EM
    counts, codes, ls, pairs = input_case(20)
    off, part = EM._partner_lists(pairs, 80)
    out = np.zeros((20, 80), order="F")

    def call(codes=codes, ls=ls, off=off, part=part, thr=4):
        return _lib.lib().scde_crossfit_inputs_host(None, api._p(counts), 20, 20, 80, api._p(codes), api._p(ls),
                                                    api._p(off), api._p(part), thr, 3, api._p(out), None, None)
    assert call() == 0
    bad = part.copy()
    bad[0] = 80
    other = part.copy()
    other[off[5]] = 5
    single = codes.copy()
    single[np.flatnonzero(codes == 0)[0]] = 9
    for kw, msg in (({"part": bad}, "partner"), ({"part": other}, "partner"), ({"thr": 0}, "thr"),
                    ({"ls": np.zeros(80)}, "library size"), ({"codes": single}, "single cell"),
                    ({"off": off[::-1].copy()}, "part_off")):
        with pytest.raises(_lib.ScdeError, match=msg):
            _lib.check(call(**kw))


# ------------------------------------------------------------------ 2. one round
@pytest.mark.parametrize("n,seed,kind", ONE_ROUND)
def test_one_round(n, seed, kind):
    ref = E.reference_nb2(n, seed, kind, iter=1, permutations=3)
    if kind == "underfit":
        assert ref["fit"]["refit"]
    if kind == "negative":
        assert ref["fit"]["negative_slope"] and ref["fit"]["row"][4] == 0.0
    if kind == "large":
        assert ref["cell"][0].max() >= 100000
    if kind == "sparse":
        assert int(np.sum(ref["cell"][0] > 1)) == 3
    mm, det = run([ref["cell"]], iter=1)
    check_fit(mm, det, 0, ref, f"n = {n}, seed {seed}, {kind}")


def test_one_round_400_cells_of_40_genes():
    """More cells than workgroups are resident: the groups stride over the cells."""
    cells = [E.synthetic_cell_nb2(40, 5000 + j) for j in range(400)]
    mm, det = run(cells, iter=1)
    ok = det["status"] == 0
    assert ok.sum() >= 300 and np.all(det["iterations"][ok] == 1)
    assert np.all(np.isfinite(mm[ok][:, :6])) and np.all(np.isnan(mm[~ok]))
    checked = 0
    for j in range(3, 400, 37):
        ref = E.reference_nb2(40, 5000 + j, "plain", iter=1, permutations=3)
        if not ref["stable"] or max(ref["spread"].values()) > 1e-13:
            continue  # (the choice looks at the restatement alone)
        check_fit(mm, det, j, ref, f"cell {j} of 400")
        checked += 1
    assert checked >= 5
    for j in (0, 255, 256, 399):
        alone, _ = run([cells[j]], iter=1)
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))


# ------------------------------------------------------------------ 3. the whole EM
@pytest.fixture(scope="module")
def full_em():
    refs = [E.reference_nb2(n, s, k, permutations=3) for n, s, k in FULL_EM]
    return refs, run([r["cell"] for r in refs])


@pytest.mark.parametrize("j", range(len(FULL_EM)))
def test_full_em(full_em, j):
    refs, (mm, det) = full_em
    n, seed, kind = FULL_EM[j]
    if kind == "underfit":
        assert refs[j]["fit"]["refit"]
    check_fit(mm, det, j, refs[j], f"n = {n}, seed {seed}, {kind}")


def test_full_em_list_covers_a_failure():
    refs = [E.reference_nb2(n, s, k, permutations=3) for n, s, k in FULL_EM]
    assert any(r["fit"]["status"] == E.NOT_FINITE and r["fit"]["iterations"] > 1 for r in refs)


# ------------------------------------------------------------------ 4. the same bits
def test_entries_repeat_and_agree_bit_for_bit():
    cells = [E.synthetic_cell_nb2(n, 40 + n, k) for n, k in ((65, "plain"), (257, "underfit"), (1025, "plain"),
                                                            (5, "negative"))]
    mm, det = run(cells)
    again, det2 = run(cells)
    dev, det3 = run(cells, dev=True)
    for other, d in ((again, det2), (dev, det3)):
        np.testing.assert_array_equal(bits(other), bits(mm))
        np.testing.assert_array_equal(bits(d["llh"]), bits(det["llh"]))
        np.testing.assert_array_equal(bits(d["posteriors"]), bits(det["posteriors"]))
        np.testing.assert_array_equal(d["clusters"], det["clusters"])
        np.testing.assert_array_equal(d["iterations"], det["iterations"])
        np.testing.assert_array_equal(d["status"], det["status"])
    for j in (0, 2):
        alone, da = run([cells[j]])
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))
        assert da["iterations"][0] == det["iterations"][j]
        np.testing.assert_array_equal(bits(da["posteriors"][da["rows"][0], 0]),
                                      bits(det["posteriors"][det["rows"][j], j]))


@pytest.mark.parametrize("lds_genes", [100, 3])
def test_cells_too_large_for_lds_give_the_same_bits(lds_genes):
    """With lds_genes below a cell's valid genes its vectors live in the HBM workspace."""
    cells = [E.synthetic_cell_nb2(n, 40 + n, k) for n, k in ((63, "plain"), (257, "underfit"), (1025, "plain"))]
    mm, det = run(cells, iter=3)
    ws, dws = run(cells, iter=3, lds_genes=lds_genes)
    np.testing.assert_array_equal(bits(ws), bits(mm))
    np.testing.assert_array_equal(bits(dws["posteriors"]), bits(det["posteriors"]))


def test_failed_cells_leave_the_others_alone():
    good = [E.synthetic_cell_nb2(65, 11), E.synthetic_cell_nb2(257, 12)]
    y, x, fp = E.synthetic_cell_nb2(40, 13)
    tiny = (y[:2], x[:2], fp[:2])
    none = (y[:0], x[:0], fp[:0])
    flat = (y, np.full(40, 3.0), fp)  # one magnitude: the design [1, l] is singular
    mm, det = run([good[0], tiny, flat, good[1], none], iter=4)
    assert det["status"].tolist()[:2] == [0, 1] and det["status"][3] == 0 and det["status"][4] == 1
    assert det["status"][2] in (3, 5)  # (the concomitant's Hessian fails before the IRLS can)
    for j in (1, 2, 4):
        assert np.all(np.isnan(mm[j])) and np.isnan(det["llh"][j])
        assert np.all(det["clusters"][:, j] == 0) and np.all(np.isnan(det["posteriors"][:, j]))
    for j, c in ((0, good[0]), (3, good[1])):
        alone, _ = run([c], iter=4)
        np.testing.assert_array_equal(bits(alone[0]), bits(mm[j]))


def test_fit_entry_errors():
    from scde_amd import _lib, error_models as EM
    counts, inputs, _ = pack([E.synthetic_cell_nb2(20, 1)])
    with pytest.raises(_lib.ScdeError, match="max_iter"):
        EM.nb2_fit_models(inputs, counts, iter=0)
    with pytest.raises(_lib.ScdeError, match="background_rate"):
        EM.nb2_fit_models(inputs, counts, background_rate=0.0)
    with pytest.raises(_lib.ScdeError, match="lds_genes"):
        EM.nb2_fit_models(inputs, counts, lds_genes=100000)
    with pytest.raises(ValueError):
        EM.nb2_fit_models({"fpm": inputs["fpm"][:5], "fail_prior": inputs["fail_prior"][:5]}, counts)
    rate = EM.nb2_fit_models(inputs, counts, background_rate=0.2)
    assert rate[0, 2] == math.log(0.2)


# ------------------------------------------------------------------ 5. R's own result
@pytest.fixture(scope="module")
def esmef():
    from scde_amd import error_models as EM
    import pandas as pd
    g = golden("esmef_vignette_inputs.npz")
    counts = pd.DataFrame(g["counts"], index=list(g["genes"]), columns=list(g["cells"]))
    groups = np.where(g["groups"] == 0, "ESC", "MEF")
    jmm, det = EM.scde_error_models(counts, groups=groups, linear_fit=False, return_details=True)
    return g, counts, groups, jmm, det


def test_esmef_models_against_r(esmef):
    from scde_amd.models import MODEL_COLUMNS
    g, counts, groups, jmm, det = esmef
    assert np.all(det["status"] == 0)
    assert jmm.shape == (40, 6) and list(jmm.columns) == MODEL_COLUMNS[:6]
    assert list(jmm.index) == list(g["cells"])  # (the fixture's cells are ordered by group)
    assert jmm.attrs["groups"] == list(groups)
    got, ref = np.full((40, 12), np.nan), g["models"]
    got[:, :6] = jmm.to_numpy()
    np.testing.assert_array_equal(got[:, 2], ref[:, 2])  # fail.r
    print("iterations: median", np.median(det["iterations"]), "max", det["iterations"].max())
    for name, fig in distances_to_r(got, ref).items():
        med, p90, worst = ESMEF_RESTATEMENT[name]
        print(name, "median %.3g, 90th percentile %.3g, worst %.3g" % fig)
        assert fig[0] <= 2 * med and fig[1] <= 2 * p90 and fig[2] <= 2 * worst, name


@pytest.mark.parametrize("cell", [0, 1, 25])
def test_esmef_cell_against_the_restatement(esmef, cell):
    g, counts, groups, jmm, det = esmef
    inp = det["inputs"]
    v = inp["vi"][:, cell]
    c = np.asarray(g["counts"])
    y, x, fp = c[v, cell], inp["fpm"][v, cell], inp["fail_prior"][v, cell]
    fit = E.fit_cell_nb2(y, x, fp)
    spread = {k: 0.0 for k in E.ROW_COLS}
    for s in (1, 2, 3):
        o = np.random.default_rng(s).permutation(len(y))
        p = E.fit_cell_nb2(y[o], x[o], fp[o])
        assert p["iterations"] == fit["iterations"]
        for k, d in E.row_spread(fit["row"], p["row"]).items():
            spread[k] = max(spread[k], d)
    row = jmm.to_numpy()[cell]
    got = np.full(12, np.nan)
    got[:6] = row
    fig = E.row_spread(fit["row"], got)
    tol = {k: max(FLOOR, 100 * spread[k]) for k in E.ROW_COLS}
    print(f"cell {cell}: {int(v.sum())} genes", {k: f"{d:.1e}/{tol[k]:.1e}" for k, d in fig.items()})
    assert det["iterations"][cell] == fit["iterations"] and det["status"][cell] == 0
    for k in E.ROW_COLS:
        assert fig[k] <= tol[k], k
    away = np.abs(fit["p1"] - 0.5) > 1e-6
    np.testing.assert_array_equal(det["clusters"][v, cell][away], fit["clusters"][away])


def test_esmef_inputs_and_resident_path(esmef):
    """scde_error_models fits from the inputs the first stage left on the device: the same bits
    as the two public stages called one after the other through the host."""
    from scde_amd import error_models as EM
    g, counts, groups, jmm, det = esmef
    inputs = EM.error_model_inputs(counts, groups=groups)
    for k in ("fpm", "fail_prior"):
        np.testing.assert_array_equal(bits(inputs[k]), bits(det["inputs"][k]))
    assert inputs["pairs"].shape == (2, 380)
    mm = EM.nb2_fit_models(inputs, counts)
    np.testing.assert_array_equal(bits(mm[:, :6]), bits(jmm.to_numpy()))


# ------------------------------------------------------------------ 6. linear_fit = True
def test_linear_fit_is_knn_fit_on_these_inputs(esmef):
    """No R result exists for this mode: the check is that scde_error_models feeds
    error_model_inputs' output to knn_fit_models' kernel, bit for bit."""
    from scde_amd import error_models as EM, knn
    from scde_amd.models import MODEL_COLUMNS
    g, counts, groups, _, det = esmef
    jmm, d2 = EM.scde_error_models(counts, groups=groups, linear_fit=True, return_details=True)
    assert np.all(d2["status"] == 0) and jmm.shape == (40, 12) and list(jmm.columns) == MODEL_COLUMNS
    assert np.all(jmm["corr.a"] == 1.0)
    mm = knn.knn_fit_models(det["inputs"], counts)
    np.testing.assert_array_equal(bits(jmm.to_numpy()), bits(mm))
    flat = EM.scde_error_models(counts, groups=groups, linear_fit=True, local_theta_fit=False)
    assert list(flat.columns) == [c for c in MODEL_COLUMNS if not c.startswith("corr.ltheta.")]
    mm7 = knn.knn_fit_models(det["inputs"], counts, local_theta_fit=False)[:, [0, 1, 2, 3, 4, 5, 11]]
    np.testing.assert_array_equal(bits(flat.to_numpy()), bits(mm7))


def test_nb2_fit_takes_knn_model_inputs():
    """knn.error.models with linear.fit = FALSE: fit.nb2.mixture.model on the neighbourhood stage's
    inputs."""
    from scde_amd import error_models as EM, knn
    rng = np.random.default_rng(2)
    lam = rng.gamma(0.7, 30.0, size=(400, 1)) * rng.uniform(0.5, 2.0, size=(1, 14))
    counts = np.asfortranarray((rng.poisson(lam * rng.gamma(2.0, 0.5, size=(400, 14))) *
                                (rng.random((400, 14)) < 0.7)).astype(np.int32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inputs = knn.knn_model_inputs(counts, k=5, min_nonfailed=2, min_size_entries=200)
    mm, det = EM.nb2_fit_models(inputs, counts, return_details=True)
    assert np.all(det["status"] == 0) and np.all(np.isfinite(mm[:, :6])) and np.all(np.isnan(mm[:, 6:]))
    i = 3
    v = inputs["vi"][:, i]
    fit = E.fit_cell_nb2(counts[v, i], inputs["fpm"][v, i], inputs["fail_prior"][v, i])
    assert fit["status"] == 0 and det["iterations"][i] == fit["iterations"]
    np.testing.assert_allclose(mm[i, :6], fit["row"][:6], rtol=1e-8)


# ------------------------------------------------------------------ 7. through the DE path
def test_fitted_models_through_the_de_path(esmef):
    """Counts to the DE table without R.  The differences to the run on R's stored models are
    printed, not bounded: nobody has measured them before (DESIGN.md section 4.16 records them)."""
    from scde_amd import api
    from scde_amd.prior import expression_prior
    from test_oracle import VIGNETTE_TOP6
    import pandas as pd
    g, counts, groups, jmm, det = esmef
    gser = pd.Series(pd.Categorical(groups, categories=["ESC", "MEF"]), index=list(g["cells"]))
    stored = pd.DataFrame({c: g["models"][:, j] for j, c in enumerate(jmm.columns)}, index=list(g["cells"]))
    api.set_rand("darwin")
    try:
        res = {}
        for name, models in (("fitted", jmm), ("stored", stored)):
            prior = expression_prior(models, counts, length_out=400)
            res[name] = api.scde_expression_difference(models, counts, prior, groups=gser, n_randomizations=100,
                                                       n_cores=1)
    finally:
        api.set_rand("glibc")
    a, b = res["fitted"], res["stored"]
    assert a.shape[0] == 12142
    for k in ("lb", "mle", "ub", "ce", "Z", "cZ"):
        assert np.all(np.isfinite(a[k].to_numpy())), k
    top = list(VIGNETTE_TOP6)
    print("over the vignette's six genes: largest |d mle| %.3g, largest |d Z| %.3g" % (
        np.max(np.abs(a.loc[top, "mle"] - b.loc[top, "mle"])), np.max(np.abs(a.loc[top, "Z"] - b.loc[top, "Z"]))))
    print("over all genes: largest |d mle| %.3g, largest |d Z| %.3g" % (
        np.max(np.abs(a["mle"] - b["mle"])), np.max(np.abs(a["Z"] - b["Z"]))))
