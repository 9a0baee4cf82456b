"""GPU tests of the exact t-SNE embedding (csrc/tsne.hip) against the numpy restatement of its
contract (tests/tsne_ref.py).

Inputs are well-separated Gaussian clusters (``tsne_ref.clusters``: k centres N(0, 4^2) in 10
dimensions, unit noise, label i mod k, Euclidean distance).  For the generator and seeds used
here the restatement was run on the CPU at every (n, perplexity) below: beta is equal between
float64 and long double in every row, no row ends within 1e-9 of the 1e-5 stopping threshold, a
row takes at most 21 evaluations, and at (65, 10), (129, 10), (129, 30) the 5-nearest-neighbour
label purity after 1,000 iterations is 1.0 (at n = 65 in 8 out of 8 summation orders).

Sizes.  Two block edges decide them: a gradient block is 64 points (the affinity tiles are 32),
and the row kernels, the update, the centring and the sums over blocks work in strides and blocks
of 256.  So 63, 64, 65, 129 and 255, 256, 257, 513: at 257 and 513 the strided row loops take
more than one turn and the update and centring combine the sums of several blocks.

Tolerances.  For each compared quantity E is the float64 restatement's largest error against its
own long-double evaluation of the same step, normalised by the row maximum for P and by the
array's largest magnitude for Y and uY; E is measured here for every case and the GPU must lie
within 16 E of the float64 restatement.  The factor covers another exp / log, another reduction
tree and the refined reciprocal.  Measured on the CPU (n = 63 .. 513; at n = 4, perplexity 1,
every row stops at beta = 1 with one neighbour carrying all the mass, E is 4e-99 and the device's
P must equal the restatement's to that):
    P                         E = 3.1e-16 .. 2.7e-15      bound 5.0e-15 .. 4.3e-14
    Y after one step          E = 4.3e-17 .. 2.6e-16      bound 6.9e-16 .. 4.1e-15
    uY after one step         E = 1.1e-16 .. 3.7e-16      bound 1.8e-15 .. 6.0e-15
    Y after 10 iterations     E = 7.8e-16 .. 3.6e-14      bound 1.3e-14 .. 5.8e-13
The one-step and ten-iteration comparisons start from the restatement's P (uploaded), so they
measure the iteration alone.
"""
import ctypes

import numpy as np
import pytest

import tsne_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
FACTOR = 16
PRM = (200.0, 12.0, 250, 250, 0.5, 0.8)
# T - 1, T, T + 1, 2 T + 1 for T = 64 (gradient blocks; 32: affinity tiles) and T = 256 (row
# strides, update and centring blocks), perplexities 5, 10, 30 where 3 * perplexity <= n - 1
AFFINITY_CASES = [(4, 2, 1), (63, 3, 5), (63, 3, 10), (64, 3, 5), (64, 3, 10), (65, 3, 5), (65, 3, 10), (129, 4, 5),
                  (129, 4, 10), (129, 4, 30)] + [(n, k, p) for n, k in ((255, 4), (256, 4), (257, 4), (513, 5))
                                                 for p in (5, 10, 30)]
RUN_CASES = [(65, 3, 10), (129, 4, 10), (129, 4, 30), (257, 4, 10), (513, 5, 30)]

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _input(n, k):
    return _cached(("input", n, k), lambda: R.clusters(n, k))


def _aff(n, k, perp, T=np.float64):
    return _cached(("aff", n, k, perp, T), lambda: R.affinities(R.lower_d2(_input(n, k)[0]), perp, T))


def _y0(n):
    """The seeded start.  It comes from the library's own host code (initial_Y); that it is R's
    rnorm stream is checked apart from everything here, in test_tsne.py's
    test_seeded_start_is_rnorm, against values R prints."""
    from scde_amd.embedding import initial_Y
    return _cached(("y0", n), lambda: initial_Y(n, 1))


def _trajectory(n, k, perp):
    """The float64 restatement's states at t = 0, 10, 100, 260 from the seeded start."""
    def run():
        P = _aff(n, k, perp)[0]
        st, out = R.start(_y0(n)), {}
        for t in range(261):
            if t in (0, 10, 100, 260):
                out[t] = st
            st = R.step(P, *st, t)[:3]
        return out
    return _cached(("traj", n, k, perp), run)


def _err(a, b, rowwise=False):
    """max |a - b| normalised by b's row maxima or its largest magnitude, in long double."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    scale = np.abs(b).max(1)[:, None] if rowwise else np.abs(b).max()
    return float((np.abs(a - b) / scale).max())


def _bound(ref64, refld, rowwise=False):
    return FACTOR * _err(ref64, refld, rowwise)


def _lib_():
    """(the library, the default context, the pointer helper)"""
    from scde_amd import _lib, api
    return _lib.lib(), api.default_context(), api._p


def _padded(d, pad=3):
    """The strict lower triangle of d in an (n + pad) x n buffer, NaN everywhere else."""
    n = d.shape[0]
    a = np.full((n + pad, n), np.nan, order="F")
    a[:n] = np.where(np.tri(n, k=-1, dtype=bool), d, np.nan)
    return a


def _dev_put(a):
    from scde_amd import _lib
    L, ctx, _p = _lib_()
    p = ctypes.c_void_p()
    _lib.check(L.scde_dev_alloc(ctx.handle, a.nbytes, ctypes.byref(p)))
    _lib.check(L.scde_h2d(ctx.handle, p, _p(a), a.nbytes))
    return p


def _dev_free(*ps):
    from scde_amd import _lib
    L, ctx, _ = _lib_()
    for p in ps:
        _lib.check(L.scde_dev_free(ctx.handle, p))


def _host_entry(a, ld, n, perp, max_iter=0, squared=0, Y_init=None):
    """scde_tsne_host on the buffer a: (rc, message, Y, costs, beta, P)."""
    L, ctx, _p = _lib_()
    Y, costs, beta, P = np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros((n, n), order="F")
    rc = L.scde_tsne_host(ctx.handle, _p(a), ld, n, float(perp), squared, *PRM, max_iter, 1, _p(Y_init), _p(Y),
                          _p(costs), _p(beta), _p(P))
    return rc, L.scde_last_error(), Y, costs, beta, P


def _dev_affinities(a, ld, n, perp, squared=0):
    """scde_tsne_affinities_dev on the buffer a: (rc, message, beta, P, the buffer afterwards)."""
    from scde_amd import _lib
    L, ctx, _p = _lib_()
    wsb = ctypes.c_int64()
    _lib.check(L.scde_tsne_ws_bytes(max(n, 4), ctypes.byref(wsb)))
    beta, P, after = np.zeros(n), np.full((n, n), -7.0, order="F"), np.empty_like(a)
    dp, pp, ws = _dev_put(a), _dev_put(P), ctypes.c_void_p()
    _lib.check(L.scde_dev_alloc(ctx.handle, wsb.value, ctypes.byref(ws)))
    try:
        rc = L.scde_tsne_affinities_dev(ctx.handle, dp, ld, n, float(perp), squared, pp, _p(beta), ws, wsb.value)
        msg = L.scde_last_error()
        _lib.check(L.scde_d2h(ctx.handle, _p(after), dp, a.nbytes))
        _lib.check(L.scde_d2h(ctx.handle, _p(P), pp, P.nbytes))
    finally:
        _dev_free(dp, pp, ws)
    return rc, msg, beta, P, after


def _state_on(n, k, perp, t=0):
    """A device state that holds the restatement's P and its state at iteration t."""
    from scde_amd import _lib, tsne_affinities
    L, ctx, _p = _lib_()
    st = tsne_affinities(_input(n, k)[0], perplexity=perp)
    P = np.asfortranarray(_aff(n, k, perp)[0])
    _lib.check(L.scde_h2d(ctx.handle, st._ptrs["P"], _p(P), P.nbytes))
    st.set(*_trajectory(n, k, perp)[t], t)
    return st


# ------------------------------------------------------------------ 1. affinities
@pytest.mark.parametrize("n,k,perp", AFFINITY_CASES)
def test_affinities(n, k, perp):
    d, _ = _input(n, k)
    P64, beta64, evals, dl = _aff(n, k, perp)
    Pld = _aff(n, k, perp, LD)[0]
    assert np.array_equal(_aff(n, k, perp, LD)[1].astype(np.float64), beta64) and evals.max() <= 21
    excused = np.abs(dl - 1e-5) < 1e-9
    assert excused.sum() <= 0.01 * n
    bound = _bound(P64, Pld, rowwise=True)
    a = _padded(d)
    rc, msg, Y, costs, beta_h, P_h = _host_entry(a, n + 3, n, perp)
    assert rc == 0, msg
    rc, msg, beta_d, P_d, after = _dev_affinities(a, n + 3, n, perp)
    assert rc == 0, msg
    assert after.tobytes() == a.tobytes()
    for what, beta, P in (("host", beta_h, P_h), ("dev", beta_d, P_d)):
        assert np.array_equal(beta[~excused], beta64[~excused]), what
        assert np.array_equal(P, P.T) and (np.diag(P) == 0).all(), what
        e = _err(P[~excused][:, ~excused], P64[~excused][:, ~excused], rowwise=True)
        print(f"affinities n={n} perplexity={perp} {what}: error {e:.3g}, bound {bound:.3g}")
        assert e <= bound, (what, e, bound)
        assert abs(P.sum() - 1) < 1e-12
    assert P_h.tobytes() == P_d.tobytes() and beta_h.tobytes() == beta_d.tobytes()
    # max_iter = 0: the seeded start comes back, with its cost
    assert np.array_equal(Y, _y0(n))
    c64 = R.costs(P_h, Y)
    assert np.abs(costs - c64).max() <= 1e-12 * np.abs(c64).max()


def test_squared_input():
    n, k, perp = 65, 3, 10
    d, _ = _input(n, k)
    low = np.tril(d, -1)
    rc, msg, _, _, beta, P = _host_entry(np.asfortranarray(low * low), n, n, perp, squared=1)
    assert rc == 0, msg
    ref = _host_entry(np.asfortranarray(d), n, n, perp)
    assert beta.tobytes() == ref[4].tobytes() and P.tobytes() == ref[5].tobytes()


# ------------------------------------------------------------------ 2. one step from three states
@pytest.mark.parametrize("t", [0, 100, 260])
@pytest.mark.parametrize("n,k,perp", RUN_CASES)
def test_one_step(n, k, perp, t):
    from scde_amd import tsne_iterate
    P = _aff(n, k, perp)[0]
    s0 = _trajectory(n, k, perp)[t]
    y64, u64, g64, _ = R.step(P, *s0, t)
    yld, uld, gld, _ = R.step(P.astype(LD), *(x.astype(LD) for x in s0), t, LD)
    # (the long-double gains, rounded a second time on the way to float64, may differ in the last
    # place; that both precisions took the same branch everywhere is what is checked)
    assert np.abs(gld.astype(np.float64) - g64).max() <= 2.0 ** -52 * g64.max()
    st = _state_on(n, k, perp, t)
    try:
        tsne_iterate(st, 1)
        assert st.iter == t + 1
        Y, uY, gains = np.asarray(st.Y()), st.uY(), st.gains()
    finally:
        st.close()
    assert np.array_equal(gains, g64)
    for what, got, r64, rld in (("Y", Y, y64, yld), ("uY", uY, u64, uld)):
        e, bound = _err(got, r64), _bound(r64, rld)
        print(f"one step n={n} perplexity={perp} t={t} {what}: error {e:.3g}, bound {bound:.3g}")
        assert e <= bound, (what, e, bound)


# ------------------------------------------------------------------ 3. ten iterations
@pytest.mark.parametrize("n,k,perp", RUN_CASES)
def test_ten_iterations(n, k, perp):
    from scde_amd import tsne_iterate
    P = _aff(n, k, perp)[0]
    y64 = _trajectory(n, k, perp)[10][0]
    yld = R.iterate(P, *R.start(_y0(n)), 0, 10, LD)[0]
    st = _state_on(n, k, perp, 0)
    try:
        Y = np.asarray(tsne_iterate(st, 10).Y())
    finally:
        st.close()
    e, bound = _err(Y, y64), _bound(y64, yld)
    print(f"ten iterations n={n} perplexity={perp}: error {e:.3g}, bound {bound:.3g}")
    assert e <= bound, (e, bound)


# ------------------------------------------------------------------ 4. resume, repeatability
@pytest.mark.parametrize("n,k,perp", [(65, 3, 10), (513, 5, 30)])
def test_resume_and_repeat(n, k, perp):
    from scde_amd import tsne_affinities, tsne_embedding, tsne_iterate
    d, _ = _input(n, k)
    whole = tsne_affinities(d, perplexity=perp)
    split = tsne_affinities(d, perplexity=perp)
    fresh = tsne_affinities(d, perplexity=perp)
    try:
        tsne_iterate(whole, 1000)
        tsne_iterate(split, 250)
        # 250 -> 251 on another state, resumed from what was read back
        fresh.set(split.Y(), split.uY(), split.gains(), split.iter)
        tsne_iterate(fresh, 1)
        tsne_iterate(tsne_iterate(split, 1), 749)
        tsne_iterate(fresh, 749)
        assert whole.iter == split.iter == fresh.iter == 1000
        for other in (split, fresh):
            for f in ("Y", "uY", "gains"):
                assert np.asarray(getattr(other, f)()).tobytes() == np.asarray(getattr(whole, f)()).tobytes(), f
        # a switch taken one iteration early or late would show here
        late = tsne_affinities(d, perplexity=perp, stop_lying_iter=251, mom_switch_iter=251)
        try:
            assert np.asarray(tsne_iterate(late, 251).Y()).tobytes() == _resumed_Y(d, perp, 251)
            assert np.asarray(tsne_iterate(late, 1).Y()).tobytes() != _resumed_Y(d, perp, 252)
        finally:
            late.close()
        Yd, Pd, cd = whole.Y(), whole.P(), whole.costs()
        beta_d = whole.beta
    finally:
        whole.close()
        split.close()
        fresh.close()
    one = tsne_embedding(d, perplexity=perp, return_details=True)
    two = tsne_embedding(d, perplexity=perp, return_details=True)
    for key in ("Y", "costs", "beta", "P"):
        assert one[key].tobytes() == two[key].tobytes(), key
    assert one["Y"].tobytes() == Yd.tobytes() and one["P"].tobytes() == Pd.tobytes()
    assert one["costs"].tobytes() == cd.tobytes() and one["beta"].tobytes() == beta_d.tobytes()
    assert tsne_embedding(d, perplexity=perp).tobytes() == Yd.tobytes()


def _resumed_Y(d, perp, n_iter):
    from scde_amd import tsne_affinities, tsne_iterate
    st = tsne_affinities(d, perplexity=perp)
    try:
        return np.asarray(tsne_iterate(st, n_iter).Y()).tobytes()
    finally:
        st.close()


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_65():
    from scde_amd import tsne_embedding
    n, k, perp = 65, 3, 10
    d, lab = _input(n, k)
    P = _aff(n, k, perp)[0]
    rng = np.random.default_rng(5)
    kls = []
    for r in range(8):
        perm = rng.permutation(n) if r else None
        y = R.iterate(P, *R.start(_y0(n)), 0, 1000, perm=perm)[0]
        assert R.purity(y, lab) == 1.0
        kls.append(float(R.costs(P, y).sum()))
    got = tsne_embedding(d, perplexity=perp, return_details=True)
    kl = float(got["costs"].sum())
    first = float(tsne_embedding(d, perplexity=perp, max_iter=0, return_details=True)["costs"].sum())
    print(f"end to end n=65: KL {kl:.4f} (start {first:.4f}); restatement, 8 orders: {min(kls):.4f} .. {max(kls):.4f}")
    assert R.purity(got["Y"], lab) == 1.0
    assert kl <= max(kls) + (max(kls) - min(kls))
    # the device's own terms are the restatement's on the device's P and Y
    c64 = R.costs(got["P"], got["Y"])
    assert np.abs(got["costs"] - c64).max() <= 1e-12 * np.abs(c64).max()


@pytest.mark.parametrize("perp", [10, 30])
def test_end_to_end_129(perp):
    from scde_amd import tsne_embedding
    d, lab = _input(129, 4)
    got = tsne_embedding(d, perplexity=perp, return_details=True)
    first = float(tsne_embedding(d, perplexity=perp, max_iter=0, return_details=True)["costs"].sum())
    kl = float(got["costs"].sum())
    print(f"end to end n=129 perplexity={perp}: KL {kl:.4f} (start {first:.4f})")
    assert R.purity(got["Y"], lab) == 1.0
    assert kl < 0.5 * first


# ------------------------------------------------------------------ 6. triangle, labels, the PAGODA chain
def test_triangle_and_labels():
    import pandas as pd

    from scde_amd import tsne_embedding
    n, k, perp = 65, 3, 10
    d, _ = _input(n, k)
    ref = tsne_embedding(d, perplexity=perp, max_iter=30)
    assert isinstance(ref, np.ndarray) and ref.shape == (n, 2)
    low = np.where(np.tri(n, k=-1, dtype=bool), d, np.nan)
    assert tsne_embedding(low, perplexity=perp, max_iter=30).tobytes() == ref.tobytes()
    names = [f"cell{i}" for i in range(n)]
    got = tsne_embedding(pd.DataFrame(low, index=names, columns=names), perplexity=perp, max_iter=30,
                         return_details=True)
    assert list(got["Y"].index) == names and got["labels"] == names
    assert got["Y"].to_numpy().tobytes() == ref.tobytes()


def test_pagoda_cluster_cells_distance():
    from test_hclust import _cells_varinfo

    from scde_amd import pagoda_cluster_cells, tsne_embedding
    tam, vi = _cells_varinfo()
    details = pagoda_cluster_cells(tam, vi, return_details=True)
    dist = details["distance"]
    n = dist.shape[0]
    first = tsne_embedding(dist, perplexity=10, max_iter=0, return_details=True)
    got = tsne_embedding(dist, perplexity=10, return_details=True)
    assert got["Y"].shape == (n, 2) and np.isfinite(got["Y"]).all() and np.isfinite(got["costs"]).all()
    assert got["costs"].sum() < first["costs"].sum()
    assert np.array_equal(got["P"], got["P"].T) and abs(got["P"].sum() - 1) < 1e-12


# ------------------------------------------------------------------ 7. errors
def test_refused_values():
    from scde_amd import _lib, tsne_embedding
    n = 70
    base = np.asfortranarray(R.clusters(n, 3, seed=3)[0])
    for (i, j), v in (((1, 0), np.nan), ((n - 1, n - 2), np.inf), ((40, 17), -np.inf), ((33, 32), -1e-300)):
        a = base.copy(order="F")
        a[i, j] = v
        a[j, i] = 0.5  # the upper triangle is not looked at
        rc, msg, Y, costs, beta, P = _host_entry(a, n, n, 10, max_iter=5)
        assert rc == 1 and f"row {i + 1}, column {j + 1}".encode() in msg, msg
        assert not Y.any() and not costs.any() and not beta.any() and not P.any()
        rc, msg, beta, P, after = _dev_affinities(a, n, n, 10)
        assert rc == 1 and f"row {i + 1}, column {j + 1}".encode() in msg, msg
        assert after.tobytes() == a.tobytes() and not beta.any()
        with pytest.raises(_lib.ScdeError, match="negative or not finite"):
            tsne_embedding(a, perplexity=10, max_iter=5)
    # several: the first in column-major (as.dist) order is named; an overflowing square is refused
    a = base.copy(order="F")
    a[50, 3] = a[20, 5] = a[69, 2] = np.nan
    rc, msg, *_ = _host_entry(a, n, n, 10)
    assert rc == 1 and b"row 70, column 3" in msg, msg
    a = base.copy(order="F")
    a[9, 4] = 1e200
    assert _host_entry(a, n, n, 10)[0] == 1
    # the context works on
    d, _ = _input(65, 3)
    rc, msg, _, _, beta, _ = _host_entry(np.asfortranarray(d), 65, 65, 10)
    assert rc == 0 and np.array_equal(beta, _aff(65, 3, 10)[1])


def test_refused_arguments_leave_the_state():
    from scde_amd import tsne_affinities, tsne_iterate
    L, ctx, _p = _lib_()
    d, _ = _input(65, 3)
    with pytest.raises(ValueError, match="perplexity"):
        tsne_affinities(d, perplexity=22)
    a = np.asfortranarray(d)
    assert _host_entry(a, 65, 65, 22.0)[0] == 1 and b"perplexity" in L.scde_last_error()
    assert _host_entry(a, 65, 3, 1.0)[0] == 1 and b"at least 4" in L.scde_last_error()
    assert _dev_affinities(a, 65, 65, 22.0)[0] == 1
    assert _dev_affinities(a[:3, :3].copy(order="F"), 3, 3, 1.0)[0] == 1
    st = tsne_affinities(d, perplexity=10)
    try:
        tsne_iterate(st, 3)
        before = [np.asarray(f()).tobytes() for f in (st.Y, st.uY, st.gains, st.P)]
        p = st._ptrs
        for args in ((st.iter, -1, p["ws"], st.ws_bytes), (-1, 1, p["ws"], st.ws_bytes), (st.iter, 1, None, st.ws_bytes),
                     (st.iter, 1, p["ws"], st.ws_bytes - 1)):
            rc = L.scde_tsne_iterate_dev(ctx.handle, p["P"], st.n, *st.params, args[0], args[1], p["Y"], p["uY"],
                                         p["gains"], args[2], args[3])
            assert rc == 1, args
        with pytest.raises(ValueError):
            tsne_iterate(st, -1)
        bad = (float("inf"),) + st.params[1:]
        assert L.scde_tsne_iterate_dev(ctx.handle, p["P"], st.n, *bad, st.iter, 1, p["Y"], p["uY"], p["gains"],
                                       p["ws"], st.ws_bytes) == 1
        assert st.iter == 3
        assert [np.asarray(f()).tobytes() for f in (st.Y, st.uY, st.gains, st.P)] == before
        # and it goes on: the same bits as an undisturbed run
        tsne_iterate(st, 2)
        assert np.asarray(st.Y()).tobytes() == _resumed_Y(d, 10, 5)
        zero = np.asarray(tsne_iterate(st, 0).Y()).tobytes()
        assert zero == _resumed_Y(d, 10, 5) and st.iter == 5
    finally:
        st.close()
