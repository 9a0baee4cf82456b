"""The cases of tests/ratio_edge_cases.py without a GPU: the oracle's own behaviour on them, and the
preconditions the GPU tests (tests/test_gpu_ratio_edges.py) rest on.

* the oracle's matSlideMult on every finite non-negative row against exact rational sums: each lag
  within len * 2^-53 relative (len its number of terms; plus len * 2^-1074 where products go
  subnormal, +inf allowed only where the exact sum reaches DBL_MAX within that bound), and on every
  row at n <= 9 bit-equal to a plain sequential restatement -- the reference is right on these shapes;
* the threshold rows: every running sum exact in a 64-bit significand, long double and rational
  arithmetic agree on lb / ub, the oracle returns those, and on the rows built for it a float64
  running sum picks another column -- a kernel that summed in plain double would fail;
* the oracle on the tie, not-found and one-column rows: first maximum, diffv[0], diffv[m - 1];
* zi = m - 1: the share of rows on which the reference itself returns NaN.
"""
import math
import sys
from fractions import Fraction

import numpy as np
import pytest

import ratio_edge_cases as E

L10_2 = 0.30102999566398119521  # the oracle's log10(2)
DBL_MAX = Fraction(sys.float_info.max)


def _first_max(x):
    """R's which.max: the first column that exceeds all before it, NaN never exceeding (0 if none)."""
    best, col = -math.inf, 0
    for c, v in enumerate(x):
        if v > best:
            best, col = v, c
    return col


@pytest.mark.parametrize("n", E.SLIDE_SIZES)
def test_oracle_slide_against_rational(oracle, n):
    A, B, names, kinds = E.slide_rows(n)
    ref = oracle.matSlideMult(A, B)
    assert ref.shape == (A.shape[0], 2 * n - 1)
    lens = [n - abs(o - (n - 1)) for o in range(2 * n - 1)]
    checked = 0
    for r, (name, kind) in enumerate(zip(names, kinds)):
        if kind not in E.EXACT_KINDS:
            continue
        assert np.all(np.isfinite(A[r])) and np.all(np.isfinite(B[r])) and not np.any(A[r] < 0) and not np.any(B[r] < 0)
        exact = E.exact_slide(A[r], B[r])
        for o, (ex, ln) in enumerate(zip(exact, lens)):
            got = float(ref[r, o])
            slack = ln * (ex * Fraction(1, 2 ** 53) + Fraction(1, 2 ** 1074))
            if math.isinf(got):
                assert kind == "overflow" and got > 0 and ex + slack >= DBL_MAX, (n, name, o)
                continue
            assert abs(Fraction(got) - ex) <= slack, (n, name, o, got, float(ex))
            if ex == 0:
                assert got == 0 and not math.copysign(1.0, got) < 0, (n, name, o)  # +0, never -0
        checked += 1
    assert checked >= 25


@pytest.mark.parametrize("n", [n for n in E.SLIDE_SIZES if n <= 9])
def test_oracle_slide_sequential_restatement(oracle, n):
    """All rows, the non-finite and negative ones included: X[o] = sum_t A[t + max(s, 0)] B[t + max(-s, 0)],
    s = o - (n - 1), over exactly n - |s| terms in ascending t, from +0."""
    A, B, names, _ = E.slide_rows(n)
    ref = oracle.matSlideMult(A, B)
    want = np.zeros_like(ref)
    with np.errstate(all="ignore"):
        for r in range(A.shape[0]):
            for o in range(2 * n - 1):
                s = o - (n - 1)
                acc = np.float64(0.0)
                for t in range(n - abs(s)):
                    acc = acc + A[r, t + max(s, 0)] * B[r, t + max(-s, 0)]
                want[r, o] = acc
    assert np.array_equal(ref, want, equal_nan=True)
    assert np.array_equal(np.signbit(ref), np.signbit(want))
    if n == 5:  # a lag that does not hold the infinite entry stays finite
        r = names.index("B[4]=inf")
        assert np.isfinite(ref[r, (n - 1) + 1]) and ref[r, n - 1] == np.inf


@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_threshold_rows_preconditions(oracle, m):
    rows = E.threshold_rows(m)
    diffv = E.summary_diffv(m)
    X = np.asfortranarray(np.vstack([x for _, x, _ in rows]))
    got = oracle.quick_distribution_summary(X, diffv, 0.0)
    ndiff = 0
    for r, (name, x, plain_differs) in enumerate(rows):
        assert all(Fraction(float(v)) % Fraction(1, 2 ** 60) == 0 for v in x), (m, name)
        lb, ub, exact = E.exact_bounds(x)
        assert exact, (m, name)
        assert E.longdouble_bounds(x) == (lb, ub), (m, name)
        assert got["lb"][r] == diffv[lb] / L10_2 and got["ub"][r] == diffv[ub] / L10_2, (m, name)
        if plain_differs:
            assert E.longdouble_bounds(x, np.float64) != (lb, ub), (m, name)
            ndiff += 1
    if m >= 127:
        assert ndiff >= 2 * (len(E.crossing_columns(m)) - 2)
    # the designed outcomes, where the row has room for them
    names = [n for n, _, _ in rows]
    for c in E.crossing_columns(m):
        if 1 <= c and c + 4 < m - 1:
            lb = {k: E.exact_bounds(rows[names.index(f"lb-{k}-c{c}")][1])[0] for k in ("equal", "ulp-below", "quarter")}
            assert lb["equal"] == c - 1 and lb["ulp-below"] == c and lb["quarter"] in (c + 1, c + 2), (m, c, lb)
            ub = {k: E.exact_bounds(rows[names.index(f"ub-{k}-c{c}")][1])[1] for k in ("equal", "ulp-above", "quarter")}
            assert ub["equal"] == c + 1 and ub["ulp-above"] == c and ub["quarter"] in (c + 2, c + 3), (m, c, ub)


@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_oracle_on_bound_and_tie_rows(oracle, m):
    diffv = E.summary_diffv(m)
    rows = E.bound_rows(m) + E.tie_rows(m)
    X = np.asfortranarray(np.vstack([x for _, x in rows]))
    got = oracle.quick_distribution_summary(X, diffv, 0.0)
    names = [n for n, _ in rows]
    for r, (name, x) in enumerate(rows):
        assert got["mle"][r] == diffv[_first_max(x)] / L10_2, (m, name)
    assert got["lb"][names.index("lb-not-found")] == diffv[0] / L10_2
    for nm in ("ub-not-found", "ub-not-found-flat", "all-zero", "all-nan"):
        assert got["ub"][names.index(nm)] == diffv[m - 1] / L10_2, nm
    if m >= 127:  # the ties are where the names say, and there are at least two of them
        per = E.per_thread(m)
        for nm in ("tie-two-chunks", "tie-two-waves"):
            x = rows[names.index(nm)][1]
            cols = np.nonzero(x == x.max())[0]
            assert len(cols) >= 2, (m, nm)
            if nm == "tie-two-chunks":
                assert cols[0] // per != cols[1] // per and cols[1] // per < 64
            if nm == "tie-two-waves":
                assert cols[0] // per < 64 <= cols[1] // per
    assert np.isnan(got["Z"][names.index("all-nan")]) and np.isnan(got["Z"][names.index("nan-in-the-middle")])


@pytest.mark.parametrize("m", E.SUMMARY_SIZES)
def test_expectation_column_of_z_cases(m):
    from scde_amd import api
    diffv = E.summary_diffv(m)
    for zi in E.z_columns(m) + [m - 1]:
        assert api.expectation_column(diffv, diffv[zi] * E.LOG2_10) == zi


def test_many_rows_preconditions():
    A, B, y, diffv, zi = E.many_rows()
    assert A.shape == B.shape == (E.MANY_ROWS, 3) and E.MANY_ROWS > 65536
    key = B[:, 0].astype(np.int64) * 4096 + B[:, 1].astype(np.int64)
    assert len(np.unique(key)) == E.MANY_ROWS  # every row different
    zero, nan = np.all(A == 0, axis=1), np.isnan(A).any(1) | np.isnan(B).any(1)
    r = np.arange(E.MANY_ROWS)
    assert np.array_equal(nan, r % 263 == 0) and np.all(zero[r % 257 == 0]) and zero.sum() >= 255
    # the workgroup that takes row 0 (a NaN and an all-zero A) goes on to row 65,536, an ordinary one
    assert nan[0] and zero[0] and not nan[65536] and not zero[65536]
    fin = ~nan
    assert np.all(A[fin] == np.round(A[fin])) and np.all(B[fin] == np.round(B[fin])) and A[fin].max() < 1024
    assert diffv[zi] == 0.0 and len(diffv) == 5


def test_last_column_quirk(oracle):
    """zi = m - 1 in R itself: gs + zv is 1 up to rounding and qnorm(p > 1) is NaN, so the reference's
    Z is NaN on the rows where the sum rounds above 1 and the zl branch's value elsewhere."""
    for m in (21, 129, 801):
        X = E.last_column_rows(m, 2000 if m == 21 else 200)
        diffv = E.summary_diffv(m)
        z = oracle.quick_distribution_summary(X, diffv, diffv[m - 1] * E.LOG2_10)["Z"]
        zl = np.array([min(oracle.qnorm(E.oracle_gs(x, m - 1), False), 0.0) for x in X])
        nan = np.isnan(z)
        print(f"zi = m - 1, m = {m}: the oracle's Z is NaN on {nan.sum()} of {len(z)} rows")
        np.testing.assert_array_equal(z[~nan], zl[~nan])
        if m == 21:
            assert 0 < nan.sum() < len(z)
