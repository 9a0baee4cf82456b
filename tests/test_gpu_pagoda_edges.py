"""PAGODA helper kernels (pagoda.hip) at the shapes and inputs where they can go wrong:
row counts around the 64-lane stride, degenerate (0/0) columns, pair indexing at a million
pairs with a reused output buffer, the merge join's early exits, the winsorize select path's
limits and ties, and the Poisson tail of pagoda.varnorm's weights on both of its branches.

The reference of every correlation is the numpy restatement below of the formulas in
src/pagoda.cpp, evaluated in float64 and in np.longdouble.  A GPU value must lie within

    MARGIN x (max |float64 restatement - longdouble restatement| on that case) + FLOOR

of the longdouble value, NaN exactly where the restatement has NaN (tests/test_distance.py's
bar, for the same reason: the GPU sums lane-parallel in a tree, not in numpy's order).
MARGIN = 16, FLOOR = 8 ulp of 1.  The CPU tests show, for every case the GPU tests use, that the
two restatements agree on the NaN positions and that the C oracle (oracle/pagoda_oracle.c)
meets the same bound.  winsorizeMatrix only moves values: bit-exact against the oracle, and
against np.clip to the order statistics where the two trimmed ranges do not overlap.
Measured GPU maxima per test: DESIGN.md sections 4.4 and 4.5.
"""
import numpy as np
import pytest

from oracle import pagoda as OP

MARGIN = 16.0
FLOOR = 8 * 2.0 ** -52
LD = np.longdouble

_REF = {}


def _cached(key, fn):
    """One evaluation per session, shared by the CPU and GPU tests (never modified)."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# ------------------------------------------------------------------ restatements
def ref_matwcorr(m, w, T):
    """src/pagoda.cpp:41-65 for every pair i < j at once: jw = sqrt(w_i w_j) / sum, weighted
    means removed, sum(a b jw) / sqrt(sum(a a jw) sum(b b jw)) at [j, i]; identity diagonal,
    upper triangle 0."""
    m = np.asarray(m, T)
    w = np.asarray(w, T)
    n = m.shape[1]
    out = np.zeros((n, n), T)
    out[np.arange(n), np.arange(n)] = 1
    j, i = np.tril_indices(n, -1)
    if len(i) == 0:
        return out
    with np.errstate(invalid="ignore", divide="ignore"):
        jw = np.sqrt(w[:, i] * w[:, j])
        jw = jw / jw.sum(0)
        a = m[:, i] - (m[:, i] * jw).sum(0)
        b = m[:, j] - (m[:, j] * jw).sum(0)
        out[j, i] = (a * b * jw).sum(0) / np.sqrt((a * a * jw).sum(0) * (b * b * jw).sum(0))
    return out


def ref_matcorr(x, y, T):
    """arma::cor(x, y) (src/pagoda.cpp:33-38): (x'y - sum(x)' sum(y) / k) / (k - 1) over
    sd(x)' sd(y), sd from Armadillo's corrected two-pass variance."""
    x = np.asarray(x, T)
    y = np.asarray(y, T)
    k = x.shape[0]

    def sd(v):
        t = v.sum(0) / T(k) - v
        return np.sqrt(((t * t).sum(0) - t.sum(0) ** 2 / T(k)) / T(k - 1))

    with np.errstate(invalid="ignore", divide="ignore"):
        c = (x.T @ y - np.outer(x.sum(0), y.sum(0)) / T(k)) / T(max(k - 1, 1))
        return c / np.outer(sd(x), sd(y))


def _dense(pl, ngenes, T):
    v = np.zeros((len(pl), ngenes), T)
    k = np.zeros((len(pl), ngenes), T)
    for p, (i, x) in enumerate(pl):
        v[p, i] = np.asarray(x, T)
        k[p, i] = 1
    return v, k


def ref_plcor(pl, ngenes, T):
    """src/pagoda.cpp:67-117 as a set intersection on gene masks: over the genes two lists
    share, r = sum(v1 v2) / sqrt(sum(v2^2) sum(v1^2)) (0 when that product is not positive),
    n = |union|; diagonal r = 1, n = 0.  (Zeros added for the genes not shared are exact.)"""
    v, k = _dense(pl, ngenes, T)
    l12 = v @ v.T
    sq = k @ (v * v).T          # [a, b]: sum of v_b^2 over the shared genes
    cv = sq * sq.T
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(cv > 0, l12 / np.sqrt(cv), T(0))
    ln = k.sum(1)
    n = (ln[:, None] + ln[None, :] - k @ k.T).astype(np.int64)
    d = np.arange(len(pl))
    r[d, d] = 1
    n[d, d] = 0
    return r, n.astype(np.int32)


def ref_plcor_loop(pl, T):
    """The same per pair with np.intersect1d (tests/test_gpu_pagoda.py's restatement, in T)."""
    npl = len(pl)
    r = np.eye(npl, dtype=T)
    n = np.zeros((npl, npl), np.int32)
    for a in range(npl):
        for b in range(a + 1, npl):
            ia, va = pl[a]
            ib, vb = pl[b]
            common, xa, xb = np.intersect1d(ia, ib, return_indices=True)
            va, vb = np.asarray(va, T)[xa], np.asarray(vb, T)[xb]
            cv = (vb * vb).sum() * (va * va).sum()
            r[a, b] = r[b, a] = (va * vb).sum() / np.sqrt(cv) if cv > 0 else T(0)
            n[a, b] = n[b, a] = len(ia) + len(ib) - len(common)
    return r, n


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def assert_close(got, ref, what):
    """got against the (float64, longdouble) restatement pair, the module docstring's bound.
    Returns the maximum error."""
    r64, rld = ref
    got = np.asarray(got)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    assert same_nan(r64, rld), f"{what}: the restatement is not well defined on this case"
    nan = np.isnan(rld)
    own = float(np.max(np.abs(r64 - rld)[~nan], initial=0.0))
    err = float(np.max(np.abs(got - rld)[~nan].astype(np.float64), initial=0.0))
    print(f"{what}: max err {err:.3e}, float64 restatement's own {own:.3e}, nan {int(nan.sum())}")
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
    assert err <= MARGIN * own + FLOOR, f"{what}: {err:.3e} > {MARGIN} x {own:.3e} + {FLOOR:.3e}"
    return err


# ------------------------------------------------------------------ cases
MATW_K = (1, 2, 63, 64, 65, 129)
MATW_N = (2, 5, 9)
MATW_CASES = [(k, n, z) for k in MATW_K for n in MATW_N for z in (False, True)]


def _matw_inputs(k, n, zero):
    """zero: column 1 has no weight at all and columns 2, 3 (0, 1 when n = 2) have weight on
    disjoint rows -- sqrt(w_i w_j) is 0 on every row of those pairs, so they are 0/0."""
    rng = np.random.default_rng(100 * k + n)
    if k == 1:  # dyadic values and weights: jw = 1 and m - m * 1 = 0 exactly, every pair is 0/0
        m, w = rng.integers(8, 33, (1, n)) / 8.0, 4.0 ** rng.integers(-1, 2, (1, n))
    else:
        m = rng.normal(size=(k, 2)) @ rng.normal(size=(2, n)) + rng.normal(size=(k, n))
        w = rng.uniform(0.1, 1.0, size=(k, n))
    if zero:
        a, b = (0, 1) if n == 2 else (2, 3)
        if n > 2:
            w[:, 1] = 0
        w[0::2, a] = 0
        w[1::2, b] = 0
    return m, w


def _matw_ref(k, n, zero):
    m, w = _matw_inputs(k, n, zero)
    return _cached(("matw", k, n, zero), lambda: (ref_matwcorr(m, w, np.float64), ref_matwcorr(m, w, LD)))


def _matw_expected_nan(k, n, zero):
    nan = np.zeros((n, n), bool)
    if k == 1:
        nan[np.tril_indices(n, -1)] = True
    elif zero and n == 2:
        nan[1, 0] = True
    elif zero:
        nan[1, 0] = nan[2:, 1] = nan[3, 2] = True
        if k == 2:  # columns 2 and 3 have weight on one row only: a single point, 0/0 with any column
            nan[2, :2] = nan[3:, 2] = nan[3, :3] = nan[4:, 3] = True
    return nan


MATC_K = (2, 3, 63, 65, 129)
MATC_N = ((1, 1), (5, 3), (9, 4))
MATC_CASES = [(k, nx, ny, z) for k in MATC_K for nx, ny in MATC_N for z in (False, True)]


def _matc_inputs(k, nx, ny, zero):
    """zero: the last column of x and the first of y are all zero (sd = 0 and covariance 0:
    0/0 in every arithmetic).  That is the only kind of constant column used: any other
    constant gives a rounding-level sd and covariance, NaN or +-inf depending on the
    summation order -- which is why cluster.py drops constant rows before it correlates."""
    rng = np.random.default_rng(1000 * k + 10 * nx + ny)
    x = rng.normal(size=(k, nx))
    y = 0.5 * x[:, np.arange(ny) % nx] + rng.normal(size=(k, ny))
    if zero:
        x[:, nx - 1] = 0
        y[:, 0] = 0
    return x, y


def _matc_ref(k, nx, ny, zero):
    x, y = _matc_inputs(k, nx, ny, zero)
    return _cached(("matc", k, nx, ny, zero), lambda: (ref_matcorr(x, y, np.float64), ref_matcorr(x, y, LD)))


PL_GENES = 12


def _pl_special():
    """Seven lists: empty; a list; its copy; one disjoint from it; two single genes (one shared
    with the list, one not); a list whose last gene precedes the first list's later genes."""
    a = (np.array([2, 5, 7, 9]), np.array([0.5, -1.25, 2.0, 0.75]))
    return [(np.zeros(0, int), np.zeros(0)), a, (a[0].copy(), a[1].copy()),
            (np.array([1, 3, 4]), np.array([1.5, -0.5, 0.25])), (np.array([5]), np.array([-3.0])),
            (np.array([6]), np.array([2.5])), (np.array([0, 2, 5]), np.array([1.0, 0.3, -0.7]))]


def _pl_random(rng, np_, kmax):
    pl = []
    for _ in range(np_):
        k = int(rng.integers(0, kmax + 1))
        pl.append((np.sort(rng.choice(PL_GENES, size=k, replace=False)), rng.normal(size=k)))
    return pl


def _pl_cases():
    """name -> lists.  np = 1 (empty and not), np = 2 for each special pair in both orders,
    np = 23 and 24 (253 / 276 pairs: one short of and past a 256-thread block)."""
    sp = _pl_special()
    cases = {"np1-empty": [sp[0]], "np1": [sp[1]]}
    for name, (p, q) in {"empty": (0, 1), "identical": (1, 2), "disjoint": (1, 3), "single-shared": (1, 4),
                         "single-apart": (1, 5), "singles": (4, 5), "ends-early": (1, 6), "both-empty": (0, 0)}.items():
        cases["np2-" + name] = [sp[p], sp[q]]
        cases["np2-" + name + "-swapped"] = [sp[q], sp[p]]
    rng = np.random.default_rng(23)
    cases["np23"] = sp + _pl_random(rng, 16, 6)
    cases["np24"] = _pl_random(rng, 17, 6) + sp
    assert [len(v) for v in cases.values()].count(23) == 1 and len(cases["np24"]) == 24
    return cases


PL_CASES = _pl_cases()


def _pl_ref(name):
    pl = PL_CASES[name]
    return _cached(("pl", name), lambda: (ref_plcor(pl, PL_GENES, np.float64), ref_plcor(pl, PL_GENES, LD)))


BIG = 1500  # 1,124,250 pairs


def _big_matw_inputs(which):
    """k = 3 rows: each column a shuffled (-1, 0, 1) plus noise, so that no weighted variance
    is small and the float64 restatement's own error stays at rounding level on every pair."""
    rng = np.random.default_rng(700 + which)
    base = np.array([-1.0, 0.0, 1.0])
    m = np.stack([rng.permutation(base) for _ in range(BIG)], axis=1) + 0.2 * rng.normal(size=(3, BIG))
    return m, rng.uniform(0.5, 1.0, size=(3, BIG))


def _big_matw_ref(which):
    m, w = _big_matw_inputs(which)
    return _cached(("bigmatw", which), lambda: (ref_matwcorr(m, w, np.float64), ref_matwcorr(m, w, LD)))


def _big_pl_inputs(which):
    return _pl_random(np.random.default_rng(900 + which), BIG, 4)


def _big_pl_ref(which):
    pl = _big_pl_inputs(which)
    return _cached(("bigpl", which), lambda: (ref_plcor(pl, PL_GENES, np.float64), ref_plcor(pl, PL_GENES, LD)))


WINS_CASES = [(2, 8193, 1), (2, 8193, 32), (3, 8192, 2458), (9, 1, 0), (9, 2, 1), (17, 4097, 5)]


def _wins_inputs(k, n, ntr):
    """Row 0: 40 copies of the row maximum and of the row minimum at scattered places (the
    ntr + 1 extremes of each side are ties, or include all the ties).  Row 1: +inf and -inf,
    and 20 copies each of the largest and smallest finite value.  Later rows: 3 ties."""
    rng = np.random.default_rng(k * 100000 + n + ntr)
    m = rng.normal(size=(k, n))
    if n >= 200:
        for row, copies in ((0, 40), (1, 20)):
            at = rng.choice(n, size=2 * copies, replace=False)
            m[row, at[:copies]] = m[row].max()
            m[row, at[copies:]] = m[row].min()
        at = rng.choice(n, size=2, replace=False)
        m[1, at[0]], m[1, at[1]] = np.inf, -np.inf
        m[2:, 7] = m[2:, n // 2] = m[2:, n - 3]
    elif n == 2:
        m[0, 1] = m[0, 0]
        m[1] = (np.inf, -np.inf)
    else:
        m[1, 0] = np.inf
        m[2, 0] = -np.inf
    return m


def _trim(n, ntr):
    trim = ntr / n
    assert int(np.floor(n * trim + 0.5)) == ntr
    return trim


def _clip_ref(m, ntr):
    s = np.sort(m, axis=1)
    n = m.shape[1]
    return np.clip(m, s[:, [ntr]], s[:, [n - ntr - 1]])


# ---- the Poisson tail: fail.r cycles over the cells through log of these
LAMBDAS = np.array([1e-3, 0.1, 1.0, 5.0, 30.0, 200.0, 1000.0])
#: 70 genes of the fixture, every sixth from the third: each cell with lambda >= 30 then meets
#: counts on both sides of its lambda (test_poisson_tail_inputs_are_usable)
TAIL_GENES = np.arange(2, 422, 6)


def _tail_inputs():
    from conftest import golden
    from oracle import oracle as O
    g = golden("esmef500.npz")
    models = {c: g["models"][:, j].copy() for j, c in enumerate(O.MODEL_COLUMNS)
              if not np.all(np.isnan(g["models"][:, j]))}
    counts = np.ascontiguousarray(g["counts"][TAIL_GENES])
    lam = LAMBDAS[np.arange(counts.shape[1]) % len(LAMBDAS)]
    models["fail.r"] = np.log(lam)
    return models, counts, {"x": g["prior_x"], "y": g["prior_y"]}, lam


def _tail_oracle():
    models, counts, prior, _ = _tail_inputs()
    return _cached(("tail",), lambda: OP.varnorm_weights(models, counts, prior["x"], n_randomizations=20, n_cores=2,
                                                         use_expected_value=False))


# ------------------------------------------------------------------ CPU tests
def _oracle_close(got, ref, what):
    assert_close(got, ref, "oracle " + what)


@pytest.mark.parametrize("k,n,zero", MATW_CASES)
def test_matwcorr_restatements_and_oracle(k, n, zero):
    m, w = _matw_inputs(k, n, zero)
    r64, rld = _matw_ref(k, n, zero)
    assert same_nan(r64, rld)
    assert np.array_equal(np.isnan(r64), _matw_expected_nan(k, n, zero))
    assert np.max(np.abs(r64 - rld)[~np.isnan(rld)], initial=0.0) < 1e-12
    got = OP.matWCorr(m, w)
    _oracle_close(got, (r64, rld), f"matWCorr k={k} n={n} zero={zero}")
    assert np.all(got[np.triu_indices(n, 1)] == 0) and np.all(np.diag(got) == 1)


@pytest.mark.parametrize("k,nx,ny,zero", MATC_CASES)
def test_matcorr_restatements_and_oracle(k, nx, ny, zero):
    x, y = _matc_inputs(k, nx, ny, zero)
    r64, rld = _matc_ref(k, nx, ny, zero)
    assert same_nan(r64, rld)
    nan = np.zeros((nx, ny), bool)
    if zero:
        nan[nx - 1, :] = nan[:, 0] = True
    assert np.array_equal(np.isnan(r64), nan)
    if not zero and k > 2:
        np.testing.assert_allclose(r64, np.corrcoef(x.T, y.T)[:nx, nx:], rtol=0, atol=1e-12)
    _oracle_close(OP.matCorr(x, y), (r64, rld), f"matCorr k={k} nx={nx} ny={ny} zero={zero}")


@pytest.mark.parametrize("name", list(PL_CASES))
def test_plcor_restatements_and_oracle(name):
    pl = PL_CASES[name]
    (r64, n64), (rld, nld) = _pl_ref(name)
    assert not np.isnan(r64).any() and not np.isnan(rld).any() and np.array_equal(n64, nld)
    # the mask form is the per-pair set intersection
    rl, nl = ref_plcor_loop(pl, LD)
    assert np.array_equal(nl, nld) and np.max(np.abs(rl - rld), initial=0.0) <= FLOOR
    got = OP.plSemicompleteCor2(pl)
    assert np.array_equal(got["n"], nld)
    _oracle_close(got["r"], (r64, rld), "plSemicompleteCor2 " + name)


def test_plcor_special_pairs_have_the_expected_values():
    """What the special lists are for: identical r = 1 (n = its length), disjoint r = 0 exactly
    (n = the sum), an empty list r = 0 and n = the other's length."""
    for name, r, n in (("np2-identical", 1.0, 4), ("np2-disjoint", 0.0, 7), ("np2-empty", 0.0, 4),
                       ("np2-single-apart", 0.0, 5), ("np2-single-shared", 1.0, 4), ("np2-both-empty", 0.0, 0)):
        for nm in (name, name + "-swapped"):
            got = OP.plSemicompleteCor2(PL_CASES[nm])
            assert got["n"][0, 1] == got["n"][1, 0] == n, nm
            assert got["r"][0, 1] == got["r"][1, 0], nm
            assert got["r"][0, 1] == r if r == 0.0 else abs(got["r"][0, 1] - r) <= FLOOR, nm


def test_big_pair_references_and_oracle():
    """The million-pair cases: both restatements defined everywhere, the oracle within the bound,
    and the two data sets different at nearly every pair (so a stale value shows)."""
    refs = [_big_matw_ref(w) for w in (0, 1)]
    for w in (0, 1):
        r64, rld = refs[w]
        assert not np.isnan(r64).any() and not np.isnan(rld).any()
        assert np.max(np.abs(r64 - rld)) < 1e-12
        _oracle_close(OP.matWCorr(*_big_matw_inputs(w)), refs[w], f"matWCorr 3 x {BIG} #{w}")
    low = np.tril_indices(BIG, -1)
    assert np.mean(np.abs(refs[0][1] - refs[1][1])[low] > 1e-6) > 0.99
    prefs = [_big_pl_ref(w) for w in (0, 1)]
    for w in (0, 1):
        (r64, n64), (rld, nld) = prefs[w]
        got = OP.plSemicompleteCor2(_big_pl_inputs(w))
        assert np.array_equal(got["n"], nld) and np.array_equal(n64, nld)
        _oracle_close(got["r"], (r64, rld), f"plSemicompleteCor2 {BIG} #{w}")
    assert np.mean((prefs[0][1][1] != prefs[1][1][1])[low]) > 0.5


@pytest.mark.parametrize("k,n,ntr", WINS_CASES)
def test_oracle_winsorize_edges_against_clip(k, n, ntr):
    m = _wins_inputs(k, n, ntr)
    got = OP.winsorizeMatrix(m, _trim(n, ntr))
    if 2 * ntr < n:
        np.testing.assert_array_equal(got, _clip_ref(m, ntr))
        if n >= 200 and ntr:
            assert (got != m).any() and np.isinf(m[1]).sum() == 2 and not np.isinf(got[1]).any()
    else:  # n = 2, ntr = 1: each row's two values change places
        np.testing.assert_array_equal(got, m[:, ::-1])


def test_winsorize_select_refuses_more_than_32():
    """Rows longer than the LDS sort take the select kernel, which holds 33 extremes per side;
    round(ncol * trim) = 33 is refused before a device is looked for."""
    from scde_amd import pagoda as PG
    from scde_amd._lib import ScdeError
    with pytest.raises(ScdeError, match=r"scde_hip error 1: winsorizeMatrix: ncol > 8192 needs round\(ncol \* trim\) <= 32"):
        PG.winsorizeMatrix(np.zeros((2, 8193)), _trim(8193, 33))


def test_poisson_tail_inputs_are_usable():
    """fail.r = log(lambda) replaced per cell: (1) each row of the oracle's joint posterior has
    its maximum more than 1e-6 relative (the posterior bar) above the runner-up, so the grid
    mode cannot flip; (2) the cells with lambda = 30, 200, 1000 meet counts in [1, lambda) and
    counts >= lambda, the two branches of the tail."""
    from oracle import oracle as O
    models, counts, prior, lam = _tail_inputs()
    jp = O.scde_posteriors(models, counts, prior["x"], n_randomizations=20, n_cores=2)
    s = np.sort(jp, axis=1)
    assert np.all(s[:, -1] - s[:, -2] > 1e-6 * s[:, -1])
    assert set(lam.tolist()) == set(LAMBDAS.tolist())
    for j in np.nonzero(lam >= 30)[0]:
        col = counts[:, j]
        assert ((col >= 1) & (col < lam[j])).any() and (col >= lam[j]).any(), (j, lam[j])
    want = _tail_oracle()
    assert np.all(np.isfinite(want["matw"])) and want["matw"].min() >= 0 and want["matw"].max() <= 1


# ------------------------------------------------------------------ GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("k,n,zero", MATW_CASES)
def test_matwcorr_row_counts_and_zero_weights(k, n, zero):
    from scde_amd import pagoda as PG
    got = PG.matWCorr(*_matw_inputs(k, n, zero))
    assert_close(got, _matw_ref(k, n, zero), f"matWCorr k={k} n={n} zero={zero}")
    assert np.all(got[np.triu_indices(n, 1)] == 0) and np.all(np.diag(got) == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("k,nx,ny,zero", MATC_CASES)
def test_matcorr_row_counts_and_zero_columns(k, nx, ny, zero):
    from scde_amd import pagoda as PG
    got = PG.matCorr(*_matc_inputs(k, nx, ny, zero))
    assert_close(got, _matc_ref(k, nx, ny, zero), f"matCorr k={k} nx={nx} ny={ny} zero={zero}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PL_CASES))
def test_plcor_edges(name):
    from scde_amd import pagoda as PG
    got = PG.plSemicompleteCor2(PL_CASES[name])
    (r64, _), (rld, nld) = _pl_ref(name)
    np.testing.assert_array_equal(got["n"], nld)
    assert_close(got["r"], (r64, rld), "plSemicompleteCor2 " + name)
    assert np.array_equal(got["r"], got["r"].T)


@pytest.mark.gpu
def test_matwcorr_pair_indexing_at_a_million_pairs():
    """k_eye leaves the lower triangle alone and the output buffer is reused between calls: a
    pair that tri_pair skips keeps the previous call's value there, one it maps twice leaves
    another stale.  Two calls of one shape on different data; the second must be the second's."""
    from scde_amd import pagoda as PG
    first = PG.matWCorr(*_big_matw_inputs(0))
    got = PG.matWCorr(*_big_matw_inputs(1))
    ra, rb = _big_matw_ref(0), _big_matw_ref(1)
    assert_close(first, ra, f"matWCorr 3 x {BIG}, first call")
    assert_close(got, rb, f"matWCorr 3 x {BIG}, second call")
    bar = MARGIN * float(np.max(np.abs(rb[0] - rb[1]))) + FLOOR
    differ = np.abs(ra[1] - rb[1]).astype(np.float64) > bar
    assert differ[np.tril_indices(BIG, -1)].mean() > 0.99
    assert not np.any((got == first) & differ)


@pytest.mark.gpu
def test_plcor_pair_indexing_at_a_million_pairs():
    from scde_amd import pagoda as PG
    PG.plSemicompleteCor2(_big_pl_inputs(0))
    got = PG.plSemicompleteCor2(_big_pl_inputs(1))
    (r64, _), (rld, nld) = _big_pl_ref(1)
    np.testing.assert_array_equal(got["n"], nld)
    assert_close(got["r"], (r64, rld), f"plSemicompleteCor2 {BIG}")
    want = OP.plSemicompleteCor2(_big_pl_inputs(1))
    np.testing.assert_array_equal(got["n"], want["n"])
    assert float(np.max(np.abs(got["r"] - want["r"]))) <= MARGIN * float(np.max(np.abs(r64 - rld))) + FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,ntr", WINS_CASES)
def test_winsorize_edges(k, n, ntr):
    from scde_amd import pagoda as PG
    m = _wins_inputs(k, n, ntr)
    got = PG.winsorizeMatrix(m, _trim(n, ntr))
    np.testing.assert_array_equal(got, OP.winsorizeMatrix(m, _trim(n, ntr)))
    if 2 * ntr < n:
        np.testing.assert_array_equal(got, _clip_ref(m, ntr))


@pytest.mark.gpu
def test_varnorm_weights_poisson_tail_on_both_branches():
    """matw = 1 - mfp * sfp with sfp = P(X >= count), X ~ Poisson(exp(fail.r)), against
    scipy's survival function, for exp(fail.r) from 1e-3 to 1000.  Before the lower sum was
    taken relative to its largest term, exp(-1000) underflowed and every count in [1, 1000)
    of a lambda = 1000 cell got sfp = 1."""
    from scde_amd import api
    from scde_amd import pagoda as PG
    models, counts, prior, lam = _tail_inputs()
    want = _tail_oracle()
    api.set_rand("glibc")
    got = PG.pagoda_varnorm_weights(models, counts, prior, n_cores=2, n_randomizations=20, use_expected_value=False)
    np.testing.assert_array_equal(got["avmodes"], want["modes"][0])
    for lv in LAMBDAS:
        cells = np.nonzero(lam == lv)[0]
        a, b = got["matw"][:, cells], want["matw"][:, cells]
        print(f"lambda {lv:g}: max |matw - oracle| {np.max(np.abs(a - b)):.3e}")
    for lv in LAMBDAS:
        cells = np.nonzero(lam == lv)[0]
        np.testing.assert_allclose(got["matw"][:, cells], want["matw"][:, cells], rtol=1e-12, atol=1e-15,
                                   err_msg=f"lambda = {lv:g}")
