"""Inputs that drive the ratio-posterior and summary kernel (k_ratio_summary, scde_amd/csrc/ratio.hip)
through the branches it takes on VALUES, for tests/test_ratio_edges.py (CPU: the oracle on them, and
the cases' own preconditions) and tests/test_gpu_ratio_edges.py (the HIP path against the oracle).
Plain numpy; nothing here needs a GPU or the oracle.

  slide    rows for matSlideMult at each n of SLIDE_SIZES: zeros, single entries, supports at every
           residue mod 4, supports that do not meet, -0.0, products that underflow or overflow,
           negative entries, +inf and NaN (slide_rows);
  many     more rows than the launch has workgroups, n = 3 (many_rows);
  summary  rows for quick.distribution.summary at each m of SUMMARY_SIZES: cumulative sums that meet
           0.025 and 0.975 exactly, one ulp away, or only through quarter-ulp terms, with the crossing
           column at the chunk and wave boundaries of the 128-thread block; bounds that are not
           found; ties of the maximum; all mass on one column around the expectation column
           (threshold_rows, bound_rows, tie_rows, onehot_rows, last_column_rows).
"""
import math
from fractions import Fraction

import numpy as np

SLIDE_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 33, 64, 65, 401, 403)
SUMMARY_SIZES = (1, 3, 5, 127, 129, 255, 257, 801, 1601)
BLOCK = 128  # threads of a k_ratio_summary workgroup: thread t walks columns [t * per, (t + 1) * per)
MANY_ROWS = 65536 + 130  # the launch is capped at 65,536 workgroups
LOG2_10 = math.log2(10.0)

#: kinds of slide rows: "plain" (finite, >= 0, products in the normal range), "underflow",
#: "overflow" (finite, >= 0), "negative", "nonfinite"
EXACT_KINDS = ("plain", "underflow", "overflow")


def per_thread(m):
    return (m + BLOCK - 1) // BLOCK


# ------------------------------------------------------------------ slide rows
def _ks(n):
    return sorted({k for k in (0, 1, 2, 3, 4, n // 2, n - 2, n - 1) if 0 <= k < n})


def _supports(n):
    """[lo, hi] with lo and hi at every residue mod 4 (every pair of them below n = 8)."""
    if n < 8:
        return [(lo, hi) for lo in range(n) for hi in range(lo, n)]
    out = []
    for lr in range(4):
        for hr in range(4):
            lo = lr + (4 if n >= 16 else 0) + (8 * hr if n >= 64 else 0)
            hi = min(n - 1, lo + 9 + 4 * lr if n >= 64 else n - 1)
            hi -= (hi - hr) % 4
            if hi >= lo:
                out.append((lo, hi))
    out.append((n - 6, n - 1))
    out.append((n - 7, n - 2))
    return sorted(set(out))


def slide_rows(n):
    """(A, B, names, kinds): nrows x n Fortran-ordered inputs of matSlideMult, one launch."""
    rng = np.random.default_rng(1000 + n)
    A, B, names, kinds = [], [], [], []

    def dense(power=1):
        return (0.05 + rng.random(n)) ** power

    def add(name, a, b, kind="plain"):
        A.append(np.asarray(a, np.float64).copy())
        B.append(np.asarray(b, np.float64).copy())
        names.append(name)
        kinds.append(kind)

    z = np.zeros(n)
    add("dense", dense(), dense(3))
    add("A=0", z, dense())
    add("B=0", dense(), z)
    add("both=0", z, z)
    for k in _ks(n):
        e = z.copy()
        e[k] = 0.75 + 0.01 * k
        add(f"A=e{k}", e, dense())
        add(f"B=e{k}", dense(), e)
        add(f"A=e{k},B=e{n - 1 - k}", e, e[::-1].copy())
    for lo, hi in _supports(n):
        a = dense()
        a[:lo] = 0
        a[hi + 1:] = 0
        add(f"A[{lo},{hi}]", a, dense())
        add(f"B[{lo},{hi}]", dense(), a * 0.5)
        b = dense()
        b[:n - 1 - hi] = 0
        b[n - lo:] = 0
        add(f"A[{lo},{hi}],B mirrored", a, b)
    # supports at opposite ends: whole lags are exactly zero
    q = max(1, n // 4)
    first, last = dense(), dense()
    first[q:] = 0
    last[:n - q] = 0
    add("A first quarter, B last", first, last)
    add("A last quarter, B first", last, first)
    if n >= 3:
        add("A=e0,B=e(n-1)", np.eye(1, n, 0)[0], np.eye(1, n, n - 1)[0] * 0.3)
        add("A=e(n-1),B=e0", np.eye(1, n, n - 1)[0] * 0.3, np.eye(1, n, 0)[0])
    # every other entry zero inside a support
    a, b = dense(), dense()
    a[1::2] = 0
    b[::2] = 0
    add("A odd=0", a, dense())
    add("B even=0", dense(), b)
    add("A odd=0,B even=0", a, b)
    add("A odd=0,B odd=0", a, np.where(np.arange(n) % 2 == 1, 0.0, dense()))
    # -0.0
    a, b = dense(), dense()
    a[::3] = -0.0
    b[1::3] = -0.0
    add("A -0.0", a, dense())
    add("B -0.0", dense(), b)
    add("A,B -0.0", a, b)
    add("A all -0.0", np.full(n, -0.0), dense())
    add("A all -0.0, B all -0.0", np.full(n, -0.0), np.full(n, -0.0))
    # subnormal entries and products that underflow (partly, wholly)
    add("tiny*tiny -> subnormal", dense() * 1e-160, dense() * 1e-160, "underflow")
    add("tiny*tiny -> 0", dense() * 1e-170, dense() * 1e-170, "underflow")
    add("subnormal A", np.arange(1, n + 1) * 5e-324, dense(), "underflow")
    add("subnormal A, B", np.arange(1, n + 1) * 5e-324, np.arange(n, 0, -1) * 5e-324, "underflow")
    sub = dense()
    sub[::2] = 3e-310
    add("subnormal entries among normal", sub, dense(3), "underflow")
    # products that overflow to +inf
    add("1e300*1e300", dense() * 1e300, dense() * 1e300, "overflow")
    big = dense()
    big[n // 2] = 1e300
    add("one 1e300 each", big, big[::-1].copy() if n > 1 else big, "overflow")
    add("sum overflows", np.full(n, 1e154), np.full(n, 1.7e154), "overflow")
    # negative entries
    add("A negative", dense() - 0.5, dense(), "negative")
    add("B negative", dense(), dense() - 0.5, "negative")
    add("A one negative", np.where(np.arange(n) == n // 2, -1.0, dense()), dense(), "negative")
    add("A negative, B sparse", dense() - 0.5, np.where(np.arange(n) % 2 == 0, dense(), 0.0), "negative")
    # +inf and NaN
    for v, vn in ((np.inf, "inf"), (np.nan, "nan")):
        for k in sorted({0, n // 2, n - 1}):
            a, b = dense(), dense()
            a[k] = v
            add(f"A[{k}]={vn}", a, dense(), "nonfinite")
            b[k] = v
            add(f"B[{k}]={vn}", dense(), b, "nonfinite")
            add(f"A[{k}]=B[{k}]={vn}", a, b, "nonfinite")
            sp = np.where(np.arange(n) % 2 == 1, dense(), 0.0)
            add(f"A[{k}]={vn}, B sparse", a, sp, "nonfinite")
            add(f"B[{k}]={vn}, A=0", z, b, "nonfinite")
    A = np.asfortranarray(np.vstack(A))
    B = np.asfortranarray(np.vstack(B))
    return A, B, names, kinds


def slide_prior(n):
    rng = np.random.default_rng(77 + n)
    return {"x": np.linspace(0.0, 5.0, n) if n > 1 else np.array([0.0]), "y": 0.5 + rng.random(n)}


def _ints(row):
    """The doubles of a finite row as integers over a common power of two: (ints, shift) with
    row[i] == ints[i] / 2**shift exactly."""
    fr = [Fraction(float(v)) for v in row]
    shift = max([f.denominator.bit_length() - 1 for f in fr] + [0])
    return [int(f * (1 << shift)) for f in fr], shift


def exact_slide(a, b):
    """matSlideMult of one pair of finite rows in exact rational arithmetic: 2n - 1 Fractions."""
    n = len(a)
    ai, sa = _ints(a)
    bi, sb = _ints(b)
    out = [0] * (2 * n - 1)
    nzb = [(j, v) for j, v in enumerate(bi) if v]
    for i, va in enumerate(ai):
        if va:
            for j, vb in nzb:
                out[i - j + n - 1] += va * vb
    den = 1 << (sa + sb)
    return [Fraction(v, den) for v in out]


# ------------------------------------------------------------------ more rows than workgroups
def many_rows():
    """(A, B, prior_y, diffv, zi): MANY_ROWS x 3 rows of small integers (every product, lag and
    row sum exact in double, so nothing depends on a rounding), every row different; every 257th
    row all zero in A, every 263rd row with a NaN."""
    rng = np.random.default_rng(65536)
    r = np.arange(MANY_ROWS)
    A = rng.integers(1, 1024, (MANY_ROWS, 3)).astype(np.float64)
    B = rng.integers(1, 1024, (MANY_ROWS, 3)).astype(np.float64)
    B[:, 0] = r % 1019 + 1
    B[:, 1] = r // 1019 + 1  # (B[:, 0], B[:, 1]) names the row
    A[::257] = 0.0
    nan_rows = r[::263]
    B[nan_rows, 2] = np.nan
    A[nan_rows[1::2], nan_rows[1::2] % 3] = np.nan
    return (np.asfortranarray(A), np.asfortranarray(B), np.array([1.0, 2.0, 0.5]),
            np.array([-2.0, -1.0, 0.0, 1.0, 2.0]), 2)


# ------------------------------------------------------------------ summary rows
def summary_diffv(m):
    return (np.arange(m) - (m - 1) // 2) * 0.0125


def crossing_columns(m):
    """A thread's first and last column (threads 0, 5 and the last one that has columns), and the
    two columns either side of the boundary between the block's two waves."""
    per = per_thread(m)
    last_thread = (m - 1) // per
    cand = [0, per - 1, 5 * per, 6 * per - 1, 64 * per - 1, 64 * per, last_thread * per, m - 1]
    return sorted({c for c in cand if 0 <= c < m})


def _mass_row(m, c, head, at_c, extra, extra_val, tail):
    """head at column 0 (when c > 0; else folded into at_c), at_c at the crossing column, `extra`
    entries of extra_val after it, and -- with `tail`, where a column is left -- 0.96 on the last
    column (a multiple of 2^-53: the total, 0.985, passes 0.975 and is still exact)."""
    x = np.zeros(m)
    if c > 0:
        x[0] = head
        x[c] = at_c
    else:
        x[0] = head + at_c
    k = 0
    while k < extra and c + 1 + k < m:
        x[c + 1 + k] = extra_val
        k += 1
    if tail and c + 1 + k < m:
        x[m - 1] = 0.96
    return x, k


def threshold_rows(m):
    """[(name, row, plain_differs)]: rows whose running sums are all exact in a 64-bit significand
    (entries are multiples of 2^-60 and the sums stay below 2), at both thresholds.  plain_differs
    marks the rows built so that a float64 running sum picks another column than the exact one."""
    lo_t, hi_t = 0.025, 1 - 0.025
    assert hi_t == 0.975
    lo_ulp, hi_ulp = 2.0 ** -58, 2.0 ** -53
    assert np.nextafter(lo_t, 0) == lo_t - lo_ulp and np.nextafter(hi_t, 1) == hi_t + hi_ulp
    out = []
    for c in crossing_columns(m):
        # 0.025: lb is the last column whose running sum is < 0.025
        h = 2.0 ** -10
        x, _ = _mass_row(m, c, h, lo_t - h, 0, 0.0, True)
        out.append((f"lb-equal-c{c}", x, False))
        x, _ = _mass_row(m, c, h, (lo_t - lo_ulp) - h, 1, lo_ulp, True)
        out.append((f"lb-ulp-below-c{c}", x, False))
        x, k = _mass_row(m, c, h, (lo_t - lo_ulp) - h, 4, 2.0 ** -60, False)
        out.append((f"lb-quarter-c{c}", x, k == 4))
        # 0.975: ub is the first column whose running sum is > 0.975
        h = 0.5
        x, _ = _mass_row(m, c, h, hi_t - h, 1, hi_ulp, False)
        out.append((f"ub-equal-c{c}", x, False))
        x, _ = _mass_row(m, c, h, (hi_t + hi_ulp) - h, 0, 0.0, False)
        out.append((f"ub-ulp-above-c{c}", x, False))
        x, k = _mass_row(m, c, h, hi_t - h, 4, 2.0 ** -55, False)
        out.append((f"ub-quarter-c{c}", x, k == 4 and c + 4 < m - 1))
    return out


def bound_rows(m):
    """lb not found (no running sum below 0.025: diffv[0]); ub not found (total below 0.975:
    diffv[m - 1])."""
    a = np.zeros(m)
    a[0] += 0.5
    a[m - 1] += 0.5
    b = np.zeros(m)
    b[m // 2] = 0.5
    c = np.full(m, 0.9 / m)
    return [("lb-not-found", a), ("ub-not-found", b), ("ub-not-found-flat", c)]


def tie_rows(m):
    """Ties of the maximum: in two threads' chunks, in the two waves, within one chunk; an all-equal,
    an all-zero and an all-NaN row; a NaN in the middle.  Backgrounds are multiples of 2^-30 below
    the tied value."""
    rng = np.random.default_rng(500 + m)
    per = per_thread(m)
    top = 0.25

    def back():
        return rng.integers(0, 1 << 20, m) * 2.0 ** -30

    def tied(cols):
        cols = sorted({c for c in cols if 0 <= c < m})
        x = back()
        x[cols] = top
        return x

    out = [("tie-two-chunks", tied([2 * per, 9 * per + per - 1])),
           ("tie-two-waves", tied([3 * per + per // 2, 64 * per])),
           ("tie-second-wave-first", tied([64 * per + 1, 64 * per + per, 70 * per])),
           ("tie-one-chunk", tied([2 * per, 2 * per + per - 1, 2 * per + per // 2])),
           ("tie-last-columns", tied([m - 1, m - 2])),
           ("all-equal", np.full(m, 2.0 ** -11)),
           ("all-zero", np.zeros(m)),
           ("all-nan", np.full(m, np.nan))]
    # (a reduction that kept either of two equal maxima would still be right on ties whose lanes
    # it happens to visit in order: neighbouring threads 1 and 2, and random sets of columns)
    out.append(("tie-threads-1-2", tied([per, 2 * per])))
    for i in range(8):
        out.append((f"tie-random-{i}", tied(rng.choice(m, size=min(m, 2 + i % 5), replace=False))))
    x = tied([m // 2 + 1, m - 1, 1])
    x[m // 2] = np.nan
    out.append(("nan-in-the-middle", x))
    x = tied([m // 2 + 1, m - 1])
    x[0] = np.nan
    out.append(("nan-first", x))
    return out


def z_columns(m):
    """The expectation columns of the Z cases (zi = m - 1 has its own group)."""
    return sorted({zi for zi in (0, 1, (m - 1) // 2, m - 2) if 0 <= zi < m})


def onehot_rows(m, zi):
    cols = sorted({c for c in (0, zi - 1, zi, zi + 1, m - 1) if 0 <= c < m})
    return [(f"all-mass-c{c}", np.eye(1, m, c)[0]) for c in cols]


def summary_rows(m):
    """Every row of the summary cases at m that does not depend on zi: (names, m-column matrix)."""
    rows = [(n, x) for n, x, _ in threshold_rows(m)] + bound_rows(m) + tie_rows(m)
    return [n for n, _ in rows], np.asfortranarray(np.vstack([x for _, x in rows]))


def last_column_rows(m, nrows=200):
    """Random normalised rows for zi = m - 1, where gs + zv is 1 up to rounding and R's own Z is
    NaN whenever it rounds above."""
    rng = np.random.default_rng(900 + m)
    x = rng.random((nrows, m)) ** 4
    x /= x.sum(1, keepdims=True)
    return np.asfortranarray(x)


def ratio_inputs(m, nrows=24):
    """Two nrows x n inputs (n = (m + 1) / 2) whose normalised ratio posterior has m columns:
    peaked rows, a few with zeros, for the fused summary against the separate one."""
    n = (m + 1) // 2
    rng = np.random.default_rng(300 + m)
    g = np.arange(n)[None, :]
    c1 = rng.integers(0, n, (nrows, 1))
    c2 = rng.integers(0, n, (nrows, 1))
    w = max(1.0, n / 40.0)
    a = np.exp(-0.5 * ((g - c1) / w) ** 2) + 1e-9 * rng.random((nrows, n))
    b = np.exp(-0.5 * ((g - c2) / (2 * w)) ** 2) + 1e-9 * rng.random((nrows, n))
    a[::5, : n // 3] = 0.0
    b[1::5, n - n // 4:] = 0.0
    return np.asfortranarray(a), np.asfortranarray(b), 0.5 + rng.random(n)


# ------------------------------------------------------------------ exact restatements
def exact_bounds(x):
    """(lb column, ub column, exact) of one finite row by rational running sums: lb the last column
    with the sum, rounded to double, < 0.025 (0 if none), ub the first with it > 0.975 (m - 1 if
    none); exact: every partial sum fits a 64-bit significand."""
    lo_t, hi_t = Fraction(0.025), Fraction(1 - 0.025)
    s = Fraction(0)
    lb, ub, exact = 0, None, True
    for c, v in enumerate(x):
        s += Fraction(float(v))
        d = Fraction(float(s))  # round to nearest even, as the conversion from long double does
        num = s.numerator
        if num and (num >> ((num & -num).bit_length() - 1)).bit_length() > 64:
            exact = False
        if d < lo_t:
            lb = c
        if ub is None and d > hi_t:
            ub = c
    return lb, (len(x) - 1 if ub is None else ub), exact


def longdouble_bounds(x, dtype=np.longdouble):
    """The same through a running sum in `dtype` (the oracle's long double; float64: the plain sum)."""
    cs = np.cumsum(np.asarray(x, dtype)).astype(np.float64)
    below = np.nonzero(cs < 0.025)[0]
    above = np.nonzero(cs > 1 - 0.025)[0]
    return (int(below[-1]) if below.size else 0), (int(above[0]) if above.size else len(x) - 1)


def oracle_gs(x, zi):
    """gs of get.ratio.posterior.Z.score as the oracle forms it (long double sums of the
    pseudo-counted row), for the zi = m - 1 group."""
    p = np.asarray(x, np.float64) + 1e-15
    rs = np.float64(np.cumsum(p.astype(np.longdouble))[-1])  # (cumsum: in column order, as the oracle)
    q = (p / rs).astype(np.longdouble)
    hi = 1 if zi == 0 else zi
    return float(np.float64(np.cumsum(q[:hi])[-1]))
