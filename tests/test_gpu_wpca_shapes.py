"""Weighted PCA (wpca.hip) at the shapes no other test reaches: the K = 5..8 template
instances, coefficients in global scratch for K = 8 / 5 / 1 and at the LDS boundary, fewer
genes than components, the multi-start K = 1 kernel (k_wpca_ms1) at its cell-count and LDS
limits and with partial groups of starts, more than 8 problems of one K, and smoothing
windows that are even or longer than the gene set.

Reference and bars: the C oracle (oracle.wpca.baileyWPCA) on identical starts and
permutations, with tests/test_gpu_wpca.py's _check as it is (rotation / scores 1e-7 of the
column scale, scoreweights 1e-9, var / randvar 1e-8 relative, totvar 1e-12 relative).

A case is only usable if the reference is well conditioned on it: for every case with K >= 5
or fewer genes than components a CPU test shows that the C oracle and the independent numpy
restatement (tests/test_wpca_oracle.py's _np_round) agree to 1e-9 of the column scale on
rotation and scores, a hundredth of the GPU bar.
"""
import numpy as np
import pytest
from test_gpu_wpca import _check, _close_cols
from test_wpca_oracle import _np_round

from oracle import wpca as W

#: api_pagoda.hip, scde_bwpca_batch_dev: kLdsCap -- the EM kernel keeps the working coefficients
#: in LDS while (dmax + n) * K * sizeof(double) is at most this, else in global scratch
LDS_CAP = 160 * 1024 - 2048

_REF = {}


def _cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def _problem8(n, d, seed):
    """Rank-8 signal with singular values 3 * 0.7^r plus 0.3 noise, weights U(0.05, 1),
    columns centred by their weighted mean."""
    rng = np.random.default_rng(seed)
    L = rng.normal(size=(n, 8)) * (3.0 * 0.7 ** np.arange(8))
    m = L @ rng.normal(size=(8, d)) + 0.3 * rng.normal(size=(n, d))
    w = rng.uniform(0.05, 1.0, size=(n, d))
    return m - (m * w).sum(0) / w.sum(0), w


def _problem1(n, d, seed):
    """tests/test_gpu_configs.py::test_config5_ms1_kernel_3000_cells' rank-1 generator."""
    rng = np.random.default_rng(seed)
    m = np.outer(rng.normal(size=n), rng.normal(size=d)) * 2.0 + 0.4 * rng.normal(size=(n, d))
    w = rng.uniform(0.05, 1.0, size=(n, d))
    w[rng.uniform(size=w.shape) < 0.15] = 1e-3
    return m - (m * w).sum(0) / w.sum(0), w


def _call_case(n, d, npcs, nstarts, nsh, seed, smooth=0, gen=_problem8):
    """Inputs and oracle result of one scde_baileyWPCA call (em.tol 1e-6, 25 iterations)."""
    def make():
        m, w = gen(n, d, seed)
        K = min(npcs, d)
        starts = W.RState(seed + 1).unif_rand((1 + nsh) * nstarts * d * K)
        perms = W.shuffle_perms(seed + 2, nsh, d, n) if nsh else None
        ref = W.baileyWPCA(m, w, npcs, nstarts, smooth, 1e-6, 25, starts, nsh, perms)
        return m, w, starts, perms, ref
    return _cached(("call", n, d, npcs, nstarts, nsh, seed, smooth, gen.__name__), make)


def _gpu_call(n, d, npcs, nstarts, nsh, seed, smooth=0, gen=_problem8, what=""):
    from scde_amd import pagoda as PG
    m, w, starts, perms, ref = _call_case(n, d, npcs, nstarts, nsh, seed, smooth, gen)
    got = PG.baileyWPCA(m, w, npcs, nstarts, smooth, 1e-6, 25, 1, nsh, starts=starts, perms=perms)
    _check(got, ref, what)
    return got


# (n, d, npcs, nstarts, shuffles, seed)
BIG_K = [(70, 40, K, 2, 1, 500 + K) for K in (5, 6, 7, 8)]
#: coefficients in global scratch: K = 8 and K = 5 at n = 2600, d = 16, one start.  For K = 5
#: that shape still fits LDS ((16 + 2600) * 5 * 8 = 104,640), so n = 4100 is there as well;
#: K = 1 (the em kernel, n > 4096) needs n + d > 20,224
SCRATCH = [(2600, 16, 8, 1, 0, 610), (2600, 16, 5, 1, 0, 611), (4100, 16, 5, 1, 0, 612), (20300, 8, 1, 1, 0, 613)]
#: fewer genes than components: K = min(npcs, d); one start (with K = d the fit is exact and
#: the choice between starts would rest on rounding noise)
FEW_GENES = [(70, 1, 1, 1, 0, 620), (70, 1, 3, 1, 0, 621), (70, 2, 3, 1, 0, 622), (70, 3, 8, 1, 0, 623)]


def _in_lds(n, d, K):
    return (d + n) * K * 8 <= LDS_CAP


# ------------------------------------------------------------------ CPU: the cases are usable
@pytest.mark.parametrize("n,d,npcs,nstarts,nsh,seed", BIG_K + SCRATCH[:3] + FEW_GENES)
def test_oracle_well_conditioned_on_case(n, d, npcs, nstarts, nsh, seed):
    m, w, starts, _, ref = _call_case(n, d, npcs, nstarts, nsh, seed)
    K = min(npcs, d)
    assert ref["rotation"].shape == (d, K) and ref["scores"].shape == (n, K)
    bc, be = _np_round(m, w, nstarts, K, 25, 1e-6, starts)
    _close_cols(ref["rotation"], be, 1e-9, "rotation")
    _close_cols(ref["scores"], bc, 1e-9, "scores")
    assert np.all(np.isfinite(ref["var"])) and np.isfinite(ref["totvar"])


def test_scratch_cases_are_on_the_intended_side_of_the_cap():
    assert all(_in_lds(n, d, K) for n, d, K, *_ in BIG_K)
    assert [_in_lds(n, d, K) for n, d, K, *_ in SCRATCH] == [False, True, False, False]
    assert _in_lds(10100, 12, 2) and (12 + 10100) * 2 * 8 == LDS_CAP and not _in_lds(10100, 13, 2)


def test_nine_components_refused_before_any_device_work():
    from scde_amd import pagoda as PG
    from scde_amd._lib import ScdeError
    m, w = _problem8(70, 12, 1)
    with pytest.raises(ScdeError, match=r"scde_hip error 1: npcs must be in \[1, 8\]"):
        PG.baileyWPCA(m, w, 9, 1, 0, 1e-6, 25, 1, 0, starts=np.full(12 * 9, 0.5))


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n,d,npcs,nstarts,nsh,seed", BIG_K)
def test_five_to_eight_components(n, d, npcs, nstarts, nsh, seed):
    """k_wpca_em<K, true> / k_wpca_final<K> for K = 5..8, one shuffle (randvar)."""
    _gpu_call(n, d, npcs, nstarts, nsh, seed, what=f"K={npcs}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,npcs,nstarts,nsh,seed", SCRATCH)
def test_coefficients_in_global_scratch(n, d, npcs, nstarts, nsh, seed):
    _gpu_call(n, d, npcs, nstarts, nsh, seed, what=f"K={npcs} n={n}")


def _batch_result(res, main, shuffled=()):
    r = res[main]
    out = {k: r[k] for k in ("rotation", "scores", "scoreweights", "var", "totvar")}
    if shuffled:
        out["randvar"] = np.array([r["totvar"] - res[q]["npres1"] for q in shuffled])
    return out


def _run_single(ctx, m, w, npcs, nstarts, starts, perms=None):
    """One problem over all columns (plus one per shuffle) through DeviceMatrixPair / WpcaBatch.run."""
    from scde_amd import pagoda as PG
    n, d = m.shape
    K = min(npcs, d)
    dev = PG.DeviceMatrixPair(ctx, m.T, w.T)
    try:
        b = PG.WpcaBatch()
        per = nstarts * d * K
        b.add(np.arange(d), npcs, nstarts, starts[:per])
        nsh = 0 if perms is None else len(perms)
        for s in range(nsh):
            b.add(np.arange(d), npcs, nstarts, starts[(1 + s) * per:(2 + s) * per], perms[s])
        res = b.run(dev)
    finally:
        dev.free()
    return _batch_result(res, 0, tuple(range(1, 1 + nsh)))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [12, 13])
def test_lds_scratch_boundary(d):
    """K = 2, n = 10100: d + n = 10112 is the last size whose coefficients fit LDS_CAP."""
    from scde_amd import api
    n, K = 10100, 2
    assert _in_lds(n, d, K) == (d == 12) and (12 + n) * K * 8 == LDS_CAP
    m, w, starts, _, ref = _call_case(n, d, K, 1, 0, 630 + d)
    _check(_run_single(api.default_context(), m, w, K, 1, starts), ref, f"d + n = {d + n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,npcs,nstarts,nsh,seed", FEW_GENES)
def test_fewer_genes_than_components(n, d, npcs, nstarts, nsh, seed):
    got = _gpu_call(n, d, npcs, nstarts, nsh, seed, what=f"d={d} npcs={npcs}")
    assert got["rotation"].shape == (d, min(npcs, d))


@pytest.mark.gpu
def test_nine_components_refused_and_context_still_good():
    from scde_amd import api
    from scde_amd._lib import ScdeError
    ctx = api.default_context()
    m, w, starts, _, ref = _call_case(70, 12, 3, 2, 0, 640)
    with pytest.raises(ScdeError, match=r"scde_hip error 1: problem 0: npcs must be in \[1, 8\]"):
        _run_single(ctx, m, w, 9, 1, np.full(12 * 9, 0.5))
    _check(_run_single(ctx, m, w, 3, 2, starts), ref, "after the refusal")


@pytest.fixture(scope="module")
def ms_contexts():
    """Two private contexts: the multi-start kernel on (the default) and off."""
    from scde_amd import api
    on, off = api.Context(0), api.Context(0)
    on.set_option("wpca_ms", 1)
    off.set_option("wpca_ms", 0)
    yield on, off
    on.close()
    off.close()


def _ms_both(ms_contexts, n, d, nstarts, seed):
    m, w, starts, perms, ref = _call_case(n, d, 1, nstarts, 1, seed, gen=_problem1)
    got = [_run_single(ctx, m, w, 1, nstarts, starts, perms) for ctx in ms_contexts]
    _check(got[0], ref, f"n={n} d={d} ms on")
    _check(got[1], ref, f"n={n} d={d} ms off")
    _check(got[0], got[1], f"n={n} d={d} ms on against off")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097])
def test_ms_kernel_cell_count_edges(ms_contexts, n):
    """k_wpca_ms1<R> for R = 1..4 on both sides of each boundary, 7 starts (a group of 5 and a
    group of 2); from 4097 cells wpca_ms_ok sends K = 1 to k_wpca_em<1> whatever the option."""
    on, off = _ms_both(ms_contexts, n, 10, 7, 700 + n)
    if n > 4096:
        for key in on:
            assert np.array_equal(on[key], off[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2457, 2458])
def test_ms_kernel_lds_bound(ms_contexts, d):
    """5 starts x d doubles of E must fit 96 KiB: d = 2457 is the last gene count that does."""
    assert 2457 * 5 * 8 <= 96 * 1024 < 2458 * 5 * 8
    on, off = _ms_both(ms_contexts, 70, d, 2, 800 + d)
    if d == 2458:
        for key in on:
            assert np.array_equal(on[key], off[key]), key


def _group_batch():
    """19 K = 1 problems (nstarts 1, 5, 6, 7, 11, 3 in turn: partial trailing groups of starts,
    and unequal counts inside a group of 8 problems, hence padding blocks) and 11 K = 2
    problems over one pair; every fourth problem with a row permutation; cells 5, 60, 119
    have zero weight everywhere."""
    def make():
        n, G = 120, 90
        rng = np.random.default_rng(41)
        m = (rng.normal(size=(n, 3)) * [3.0, 1.8, 1.0]) @ rng.normal(size=(3, G)) + 0.3 * rng.normal(size=(n, G))
        w = rng.uniform(0.05, 1.0, size=(n, G))
        w[[5, 60, 119], :] = 0.0
        m = m - (m * w).sum(0) / w.sum(0)
        rs = W.RState(77)
        specs = []
        for p in range(30):
            K = 1 if p < 19 else 2
            ns = (1, 5, 6, 7, 11, 3)[p % 6] if K == 1 else 1 + p % 3
            d = int(rng.integers(12, 61))
            cols = rng.choice(G, size=d, replace=False)
            perm = W.shuffle_perms(p, 1, d, n)[0] if p % 4 == 3 else None
            st = rs.unif_rand(ns * d * K)
            mm, ww = m[:, cols], w[:, cols]
            if perm is not None:
                mm, ww = np.take_along_axis(mm, perm.T, axis=0), np.take_along_axis(ww, perm.T, axis=0)
            specs.append((cols, K, ns, st, perm, W.baileyWPCA(mm, ww, K, ns, 0, 1e-6, 25, st)))
        return m, w, specs
    return _cached(("groups",), make)


@pytest.mark.gpu
@pytest.mark.parametrize("ms", [1, 0])
def test_start_groups_and_more_than_eight_problems(ms_contexts, ms):
    from scde_amd import pagoda as PG
    m, w, specs = _group_batch()
    assert sum(K == 1 for _, K, *_ in specs) == 19 and sum(K == 2 for _, K, *_ in specs) == 11
    ctx = ms_contexts[0 if ms else 1]
    dev = PG.DeviceMatrixPair(ctx, m.T, w.T)
    try:
        b = PG.WpcaBatch()
        for cols, K, ns, st, perm, _ in specs:
            b.add(cols, K, ns, st, perm)
        res = b.run(dev)
    finally:
        dev.free()
    for p, (cols, K, ns, st, perm, ref) in enumerate(specs):
        _check(_batch_result(res, p), ref, f"problem {p} (K={K}, nstarts={ns}, ms={ms})")
        if perm is None:
            assert np.all(res[p]["scores"][[5, 60, 119]] == 0), p


@pytest.mark.gpu
@pytest.mark.parametrize("K,smooth,d", [(1, 5, 40), (3, 4, 40), (2, 9, 7)])
def test_smoothing_windows(K, smooth, d):
    """K = 1 with smoothing (forces the em kernel), an even window (L = 2 * (4 / 2) + 1 = 5),
    and a window longer than the gene set (the convolution's clipping)."""
    _gpu_call(150, d, K, 2, 0, 900 + 10 * K + smooth, smooth=smooth, what=f"K={K} smooth={smooth} d={d}")
