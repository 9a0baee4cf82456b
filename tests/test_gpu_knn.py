"""GPU tests of the neighbourhood stage of knn.error.models (csrc/knn.hip, scde_amd/knn.py)
against tests/knn_ref.py.

The comparisons are staged so that no last-bit difference can flip a discrete choice:

* the similarity against the float64 / np.longdouble pair of the restatement by the rule of
  tests/test_distance.py (MARGIN x the restatement's own error + FLOOR, NaN positions exact);
* the neighbours exactly, against the restated order applied to the implementation's own similarity;
* fpm against the restatement on the implementation's neighbours with rtol 1e-12 and NaN positions
  exact: a value is a division followed by a sum of n <= C positive terms, so any summation order
  lies within (n + 1) eps < 1e-13 of the exact mean for C <= 400;
* nabove, vi and fail_prior exactly, the last two restated from the implementation's fpm;
* the host entry against the device entry, and a call against its repetition, bit for bit.

Every test prints its figures before it asserts.
"""
import warnings

import numpy as np
import pytest

import knn_ref as R
from conftest import golden
from test_distance import FLOOR, MARGIN

pytestmark = pytest.mark.gpu

KS = (1, 5, 16, None)          # None: C - 1
TRIMS = (0.0, 0.1, 0.25, 0.5)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def synthetic(N, C, seed=0):
    """Poisson-mixture counts with about 60 % zeros; two identical cell columns (exact ties), a
    cell with no valid gene, a gene that is zero everywhere."""
    rng = np.random.default_rng(100 * N + C + seed)
    lam = rng.gamma(0.7, 12.0, size=(N, 1)) * rng.uniform(0.4, 2.5, size=(1, C))
    counts = rng.poisson(lam) * (rng.random((N, C)) < 0.45)
    counts[:, C // 3] = counts[:, 2]
    counts[:, 5] = 0
    counts[N // 2] = 0
    counts = counts.astype(np.int32)
    print(f"synthetic {N} x {C}: {np.mean(counts == 0):.2f} zeros")
    return np.asfortranarray(counts)


_cache = {}


def case(name):
    """(counts, library sizes at thr 1 and 2), built once."""
    if name not in _cache:
        if name == "knn300":
            counts, mse = np.asfortranarray(golden("knn300.npz")["counts"]), 200
        else:
            n, c = (int(v) for v in name.split("x"))
            counts, mse = synthetic(n, c), n // 2
        with np.errstate(all="ignore"):
            ls = {thr: R.estimate_library_sizes(counts, mse, thr) for thr in (1, 2)}
        counts.setflags(write=False)
        _cache[name] = (counts, ls, mse)
    return _cache[name]


def check_similarity(got, counts, thr, what):
    with np.errstate(all="ignore"):
        r64 = R.similarity(counts, thr)
        rld = R.similarity(counts, thr, dtype=np.longdouble)
    nan = np.isnan(rld)
    assert np.array_equal(np.isnan(r64), nan)
    own = float(np.max(np.abs(r64 - rld)[~nan].astype(np.float64), initial=0.0))
    err = float(np.max(np.abs(got - rld)[~nan].astype(np.float64), initial=0.0))
    print(f"{what}: gpu max err {err:.3e}, float64 restatement's own {own:.3e}, nan pairs {int(nan.sum())}")
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    assert err <= MARGIN * own + FLOOR, f"{what}: {err:.3e} > {MARGIN} x {own:.3e} + {FLOOR:.3e}"


def check_magnitudes(fpm, nabove, counts, nb, ls, thr, trim, what):
    r_fpm, r_na = R.expected_magnitudes(counts, nb, ls, thr, trim)
    nan = np.isnan(r_fpm)
    fin = np.isfinite(r_fpm)
    rel = float(np.max(np.abs(fpm[fin] - r_fpm[fin]) / np.abs(r_fpm[fin]), initial=0.0))
    print(f"{what}: fpm max rel err {rel:.3e}, NaN {int(nan.sum())} of {nan.size}, nabove max {int(r_na.max())}")
    assert np.array_equal(np.isnan(fpm), nan), f"{what}: NaN positions differ"
    assert np.array_equal(fpm[~nan & ~fin], r_fpm[~nan & ~fin]), f"{what}: infinite values differ"
    assert rel <= 1e-12, f"{what}: {rel:.3e}"
    assert nabove.dtype == np.int32 and np.array_equal(nabove, r_na), f"{what}: nabove differs"


def check_selection(res, counts, thr, min_nonfailed, min_fpm, what):
    vi = R.valid_genes(res["fpm"], res["nabove"], min_nonfailed, min_fpm)
    fp = R.fail_prior(counts, res["fpm"], vi, thr)
    nlow = [int(np.sum(counts[vi[:, i], i] <= thr)) for i in range(counts.shape[1])]
    print(f"{what}: vi genes per cell {int(vi.sum(0).min())}-{int(vi.sum(0).max())}, "
          f"cells with no low gene {sum(1 for v in nlow if v == 0)}")
    assert res["vi"].dtype == np.bool_ and np.array_equal(res["vi"], vi)
    assert np.array_equal(np.isnan(res["fail_prior"]), ~vi)
    assert np.array_equal(res["fail_prior"][vi], fp[vi])


# ------------------------------------------------------------------ the fixture, through the chain
@pytest.mark.parametrize("thr", [1, 2])
def test_model_inputs_on_the_fixture(thr):
    from scde_amd import knn
    counts, lss, mse = case("knn300")
    C = counts.shape[1]
    for k in (5, 16, 32):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = knn.knn_model_inputs(counts, k=k, min_count_threshold=thr, min_size_entries=mse)
        what = f"knn300 thr {thr} k {k}"
        assert np.array_equal(res["ls"], lss[thr])
        if k == 5:
            check_similarity(res["similarity"], counts, thr, what)
        nb = res["neighbours"]
        assert nb.shape == (C, k) and nb.dtype == np.int32
        assert np.array_equal(nb, R.neighbours(res["similarity"], k))
        check_magnitudes(res["fpm"], res["nabove"], counts, nb, res["ls"], thr, 0.25, what)
        check_selection(res, counts, thr, 5, 0, what)
        d = knn.knn_cell_data(res, counts, 3)
        g = np.flatnonzero(res["vi"][:, 3])
        assert np.array_equal(d["genes"], g) and np.array_equal(d["count"], counts[g, 3])
        assert np.array_equal(d["fpm"], res["fpm"][g, 3]) and d["cp"].shape == (len(g), 2)
        assert np.array_equal(d["cp"][:, 1], 1 - d["cp"][:, 0]) and np.array_equal(d["cp"][:, 0],
                                                                                  res["fail_prior"][g, 3])


def test_model_inputs_warns_and_takes_resident_counts():
    from scde_amd import api, knn
    counts, lss, mse = case("knn300")
    with pytest.warns(UserWarning, match="valid genes"):
        a = knn.knn_model_inputs(counts, k=16, min_size_entries=mse, min_nonfailed=12)
    assert int(a["vi"].sum(0).min()) < 40
    dc = api.DeviceCounts(api.default_context(), counts)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            b = knn.knn_model_inputs(dc, k=16, min_size_entries=mse, min_nonfailed=12)
            c = knn.knn_model_inputs(dc, k=16, library_sizes=lss[1], min_fpm=500.0)
    finally:
        dc.free()
    for key in ("ls", "similarity", "fpm", "fail_prior"):
        assert np.array_equal(bits(a[key]), bits(b[key])), key
    for key in ("neighbours", "nabove", "vi"):
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(bits(c["fpm"]), bits(a["fpm"]))
    assert 0 < c["vi"].sum() < R.valid_genes(c["fpm"], c["nabove"], 5, 0).sum()
    check_selection(c, counts, 1, 5, 500.0, "knn300 min_fpm 500")


# ------------------------------------------------------------------ synthetic counts, stage by stage
@pytest.mark.parametrize("thr", [1, 2])
@pytest.mark.parametrize("name", ["70x37", "130x130"])
def test_stages_on_synthetic_counts(name, thr):
    from scde_amd import knn
    counts, lss, _ = case(name)
    N, C = counts.shape
    ls = lss[thr]
    assert ls[5] == 0 and np.all(ls[np.arange(C) != 5] > 0)
    sim = knn.knn_cell_similarity(counts, thr)
    check_similarity(sim, counts, thr, f"{name} thr {thr}")
    assert np.isnan(sim[5]).all() and np.isnan(sim[:, 5]).all()
    for k in KS:
        kk = C - 1 if k is None else k
        nb = knn.knn_neighbours(sim, kk)
        assert nb.shape == (C, kk) and np.array_equal(nb, R.neighbours(sim, kk)), (name, thr, kk)
        others = [j for j in range(C) if j != 5]
        assert nb[5].tolist() == others[:kk]  # an all-NaN row: the first k others by index
        for trim in TRIMS:
            fpm, na = knn.knn_expected_magnitudes(counts, nb, ls, thr, trim)
            check_magnitudes(fpm, na, counts, nb, ls, thr, trim, f"{name} thr {thr} k {kk} trim {trim}")
            assert np.isnan(fpm[N // 2]).all() and not na[N // 2].any()  # the gene that is zero everywhere


@pytest.mark.parametrize("name", ["70x37", "130x130"])
def test_groups_of_unequal_size(name):
    from scde_amd import knn
    counts, lss, mse = case(name)
    N, C = counts.shape
    small = 7
    groups = np.array(["b"] * C, dtype=object)
    groups[np.arange(small) * (C // small)] = "a"   # spread over the cells, not a leading block
    k = 16                                           # above the smaller group's size - 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = knn.knn_model_inputs(counts, groups=groups, k=k, min_size_entries=mse, fpm_estimate_trim=0.1)
    nb, sim = res["neighbours"], res["similarity"]
    same = groups[:, None] == groups[None, :]
    assert np.isnan(sim[~same]).all()
    assert nb.shape == (C, k) and np.array_equal(nb, R.neighbours(sim, k, groups))
    a = np.flatnonzero(groups == "a")
    assert np.all(nb[a, small - 1:] == -1) and np.all(nb[a, :small - 1] >= 0)
    assert all(set(nb[i, :small - 1]) == set(a) - {i} for i in a)
    assert np.all(groups[nb[groups == "b"]] == "b")
    assert np.array_equal(res["ls"], lss[1])         # the library sizes are computed over all cells
    check_magnitudes(res["fpm"], res["nabove"], counts, nb, res["ls"], 1, 0.1, f"{name} groups")
    check_selection(res, counts, 1, 5, 0, f"{name} groups")
    # the standalone entry with the same groups on the whole matrix gives the same lists
    full = knn.knn_cell_similarity(counts, 1)
    assert np.array_equal(knn.knn_neighbours(full, k, groups), nb)


def test_neighbour_order_on_ties_and_nan():
    """More candidates than threads of the workgroup, values drawn from a few levels (many exact
    ties), NaN, both zeros and both infinities in the rows."""
    from scde_amd import knn
    rng = np.random.default_rng(5)
    C = 300
    levels = np.array([-np.inf, -1.0, -0.25, -0.0, 0.0, 0.125, 0.5, 1.0, np.inf, np.nan])
    sim = levels[rng.integers(0, len(levels), size=(C, C))]
    sim[7] = np.nan
    sim[8] = 0.25
    groups = rng.integers(0, 3, C)
    for k, g in ((1, None), (40, None), (C - 1, None), (500, None), (120, groups)):
        nb = knn.knn_neighbours(sim, k, g)
        ref = R.neighbours(sim, k, g)
        assert nb.shape == ref.shape and np.array_equal(nb, ref), k
        assert np.array_equal(nb, knn.knn_neighbours(sim, k, g))
    assert knn.knn_neighbours(sim).shape == (C, 150)
    assert knn.knn_neighbours(np.array([[1.0]]), 3).shape == (1, 0)
    # the default k of one cell is round(1 / 2) = 0 and of two cells 1: no error, as in R
    assert knn.knn_neighbours(np.array([[1.0]])).shape == (1, 0)
    assert knn.knn_neighbours(np.array([[1.0, 0.5], [0.5, 1.0]])).tolist() == [[1], [0]]


def test_host_and_device_entries_agree_and_repeat():
    from scde_amd import api, knn
    counts, lss, _ = case("130x130")
    N, C = counts.shape
    dc = api.DeviceCounts(api.default_context(), counts)
    try:
        s_h, s_d = knn.knn_cell_similarity(counts, 1), knn.knn_cell_similarity(dc, 1)
        assert np.array_equal(bits(s_h), bits(s_d)) and np.array_equal(bits(s_h), bits(knn.knn_cell_similarity(dc, 1)))
        nb = knn.knn_neighbours(s_h, 33)
        for trim in (0.25, 0.5):
            f_h, n_h = knn.knn_expected_magnitudes(counts, nb, lss[1], 1, trim)
            f_d, n_d = knn.knn_expected_magnitudes(dc, nb, lss[1], 1, trim)
            f_r, n_r = knn.knn_expected_magnitudes(dc, nb, lss[1], 1, trim)
            assert np.array_equal(bits(f_h), bits(f_d)) and np.array_equal(bits(f_d), bits(f_r))
            assert np.array_equal(n_h, n_d) and np.array_equal(n_d, n_r)
    finally:
        dc.free()
    # a leading dimension above the gene count
    from scde_amd._lib import check, lib
    big = np.asfortranarray(np.vstack([counts, np.full((9, C), 77, np.int32)]))
    fpm, na = np.zeros((N, C), order="F"), np.zeros((N, C), np.int32, order="F")
    check(lib().scde_knn_magnitudes_host(None, api._p(big), N + 9, N, C, api._p(nb), nb.shape[1], api._p(lss[1]), 1,
                                         0.5, api._p(fpm), api._p(na)))
    assert np.array_equal(bits(fpm), bits(f_h)) and np.array_equal(na, n_h)
    sim = np.zeros((C, C), order="F")
    check(lib().scde_knn_similarity_host(None, api._p(big), N + 9, N, C, 1, api._p(sim)))
    assert np.array_equal(bits(sim), bits(s_h))


def test_magnitudes_with_more_than_4096_cells():
    """Above 4096 cells a lane holds more than one 64-bit word of the rank mask, and the sort runs
    on 8192 entries.  Few genes and short lists keep it quick; the lists are given, so no
    similarity of this size is formed."""
    from scde_amd import knn
    rng = np.random.default_rng(11)
    N, C, kmax = 3, 4200, 70
    counts = np.asfortranarray((rng.poisson(3.0, size=(N, C)) * (rng.random((N, C)) < 0.5)).astype(np.int32))
    counts[2, :4100] = 0            # the valid values of gene 2 all rank in the second word of a lane
    counts[2, 4100:] += 1
    ls = rng.uniform(0.5, 2.0, C)
    nb = np.full((C, kmax), -1, np.int32)
    cells = rng.choice(C, 40, replace=False)
    for i in cells:
        n = int(rng.integers(1, kmax + 1))
        nb[i, :n] = rng.choice(np.delete(np.arange(C), i), n, replace=False)
    nb[cells[0], :kmax] = np.arange(4100, 4100 + kmax) + (cells[0] >= 4100) * 30
    for trim in (0.25, 0.5):
        fpm, na = knn.knn_expected_magnitudes(counts, nb, ls, 1, trim)
        r_fpm, r_na = R.expected_magnitudes(counts[:, :], nb, ls, 1, trim)
        assert np.array_equal(np.isnan(fpm), np.isnan(r_fpm)) and np.array_equal(na, r_na)
        ok = ~np.isnan(r_fpm)
        rel = float(np.max(np.abs(fpm[ok] - r_fpm[ok]) / r_fpm[ok], initial=0.0))
        print(f"4200 cells trim {trim}: {int(ok.sum())} values, max rel err {rel:.3e}")
        assert ok[:, cells].any() and rel <= 1e-12
        assert np.isnan(fpm[:, np.setdiff1d(np.arange(C), cells)]).all()  # cells without neighbours


def test_entry_errors():
    from scde_amd import api, knn
    from scde_amd._lib import ScdeError, check, lib
    counts, lss, _ = case("70x37")
    N, C = counts.shape
    L = lib()
    out = np.zeros((2, 2), np.int32)
    with pytest.raises(ScdeError, match="at most 8192"):
        check(L.scde_knn_similarity_host(None, api._p(counts), N, N, 8193, 1, api._p(np.zeros(4))))
    with pytest.raises(ScdeError, match="8192"):
        check(L.scde_knn_neighbours(None, api._p(np.zeros(4)), 8193, None, 2, 2, api._p(out)))
    with pytest.raises(ScdeError, match="kmax"):
        check(L.scde_knn_neighbours(None, api._p(np.zeros((C, C))), C, None, 5, 3, api._p(np.zeros((C, 3), np.int32))))
    nb = np.full((C, 3), -1, np.int32)
    fpm, na = np.zeros((N, C), order="F"), np.zeros((N, C), np.int32, order="F")
    for bad, msg in (((0, 1, C), "outside"), ((0, 1, -2), "outside"), ((4, 2, 9), "twice")):
        b = nb.copy()
        b[4, 0] = 9
        b[bad[0], bad[1]] = bad[2]
        with pytest.raises(ScdeError, match=msg):
            check(L.scde_knn_magnitudes_host(None, api._p(counts), N, N, C, api._p(b), 3, api._p(lss[1]), 1, 0.25,
                                             api._p(fpm), api._p(na)))
    ctx = api.Context(0)
    try:
        dc = api.DeviceCounts(api.default_context(), counts)
        try:  # resident counts with another context: refused before any call
            with pytest.raises(ValueError, match="context"):
                knn.knn_cell_similarity(dc, ctx=ctx)
            with pytest.raises(ValueError, match="context"):
                knn.knn_expected_magnitudes(dc, nb, np.ones(C), ctx=ctx)
            with pytest.raises(ValueError, match="context"):
                knn.knn_model_inputs(dc, library_sizes=np.ones(C), ctx=ctx)
        finally:
            dc.free()
        # nothing resident on a fresh context
        with pytest.raises(ScdeError, match="resident"):
            check(L.scde_knn_neighbours(ctx.handle, None, C, None, 3, 3, api._p(nb)))
        with pytest.raises(ScdeError, match="resident"):
            check(L.scde_knn_magnitudes_host(ctx.handle, api._p(counts), N, N, C, None, 3, api._p(lss[1]), 1, 0.25,
                                             api._p(fpm), api._p(na)))
    finally:
        ctx.close()
