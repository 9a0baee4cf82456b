"""Inputs that drive the posterior tables (k_tables_lpc and its fallbacks, kernels.hip) through the
branches they take on VALUES, for tests/test_table_edges.py (CPU: the oracle's own behaviour on
them) and tests/test_gpu_table_edges.py (the HIP path against the oracle).  Plain numpy.

The base case: 8 cells (rows 0..7 of the es.mef fixture's fitted models, the 6-column constant-
theta form), 140 genes whose counts give every cell 72-84 unique values -- two 64-column tasks
per cell, the second partial; the wide variant (300 genes) gives three.  A case edits ONE model
parameter of ONE cell (directly in the 12-column matrix, past the R glue's corr.a clamp), or the
magnitude grid, or the grid size:

  group F  the oracle's tables stay finite: non-positive slopes (mu not increasing: the cell is
           not "lean" and all its columns take tables_column_reg), extreme concomitant terms
           (log cfp or log(1 - cfp) = -inf), fail.r -inf / overflow, theta at the fit's limits,
           and magnitude vectors that are V-shaped, zigzag or have a plateau;
  group N  the oracle's tables of the edited cell, and hence the whole joint posterior, are NaN:
           theta inf / 0 / negative / NaN / denormal, mu = inf, fail.r NaN, and non-positive
           slopes or conc.a = 0 on the prior's own grid (first point -inf: -inf * 0);
  group W  theta far outside [1e-2, 1e3], the range the closed-form NB log-pmf was checked on;
  sizes    G at the tile, flush, wave-split and kernel-choice boundaries.
"""
import math
import os

import numpy as np

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COL = {n: j for j, n in enumerate(O.MODEL_COLUMNS)}
NCELLS = 8
NBOOT, SEED, POSTFLAG = 5, 1, 3
#: the project's bar on table values (tests/test_gpu_parity.py test_logBootPosterior_esmef)
RTOL, ATOL = 1e-11, 1e-13

_cache = {}


def _golden():
    if "g" not in _cache:
        _cache["g"] = np.load(os.path.join(GOLD, "esmef500.npz"), allow_pickle=False)
    return _cache["g"]


def base_mm():
    """The 8 x 12 model matrix of the base case (a fresh copy)."""
    M = _golden()["models"]
    models = {c: M[:NCELLS, j] for j, c in enumerate(O.MODEL_COLUMNS) if not np.all(np.isnan(M[:, j]))}
    mm, lt, sq = O.model_matrix(models)
    assert lt == 0 and sq == 0  # the constant-theta form: k_tables_lpc's path
    return mm


def counts(ngenes):
    rng = np.random.default_rng(1)
    c = rng.negative_binomial(1.0, 0.01, (ngenes, NCELLS))
    c[rng.random((ngenes, NCELLS)) < 0.3] = 0
    return np.ascontiguousarray(c.astype(np.int32))


def count_inputs(wide=False):
    """(ucl, uci) of the base case (140 genes) or the wide-counts variant (300 genes)."""
    key = ("counts", wide)
    if key not in _cache:
        ucl, uci = O.ucl_uci(counts(300 if wide else 140))
        nu = [len(u) for u in ucl]
        if wide:
            assert max(nu) >= 129, nu  # three 64-column tasks in some cell
        else:
            assert min(nu) > 64 and max(nu) <= 128, nu  # two tasks per cell, the second partial
        _cache[key] = (ucl, uci)
    return _cache[key]


def finite_grid(G):
    if G == 1:
        return np.array([1.0])
    return np.log(10.0 ** np.linspace(0.05, 5, G) - 1)


def prior_grid(G):
    """The prior's own magnitudes (first point -inf), at the fixture's 401 points or resampled."""
    x = _golden()["prior_x"]
    if G != len(x):
        x = np.linspace(x[0], x[-1], G)
    mag = O.marginals_from_prior_x(x)
    assert mag[0] == -np.inf
    return mag


def _vshape(G):
    m = finite_grid(G)
    h = G // 2
    return np.concatenate([m[h::-1], m[1:G - h]])  # descending to m[0], then ascending


def _zigzag(G):
    m = finite_grid(G).copy()
    m[1::2] -= 0.5
    return m


def _plateau(G):
    m = finite_grid(G).copy()
    m[10:20] = m[10]
    return m


MAG_SHAPES = {"vshape": _vshape, "zigzag": _zigzag, "plateau": _plateau}


class Case:
    """One call: models `mm` (cell `cell`'s parameter `col` set to `value`; `restored`: the same
    with the base value), counts and magnitudes."""

    def __init__(self, group, name, G, col=None, value=None, cell=3, mag=None, wide=False, second=None):
        self.group, self.name, self.G, self.col, self.value, self.cell, self.wide = group, name, G, col, value, cell, wide
        self.mag_kind = mag  # None: the finite grid; "prior"; or a MAG_SHAPES key
        self.second = second  # a second (col, value) edit of the same cell

    @property
    def id(self):
        return f"{self.group}-{self.name}-c{self.cell}-G{self.G}" + ("-wide" if self.wide else "")

    @property
    def edited(self):
        return self.col is not None

    def mag(self):
        if self.mag_kind is None:
            return finite_grid(self.G)
        if self.mag_kind == "prior":
            return prior_grid(self.G)
        m = MAG_SHAPES[self.mag_kind](self.G)
        assert m.shape == (self.G,) and np.all(np.isfinite(m))
        return m

    def mm(self, restored=False):
        mm = base_mm()
        if self.edited and not restored:
            mm[self.cell, COL[self.col]] = self.value
            if self.second:
                mm[self.cell, COL[self.second[0]]] = self.second[1]
        return mm

    def args(self, restored=False):
        """(mm, ucl, uci, mag, nboot, seed, postflag) of logBootPosterior."""
        ucl, uci = count_inputs(self.wide)
        return self.mm(restored), ucl, uci, self.mag(), NBOOT, SEED, POSTFLAG


def _fmt(v):
    return repr(float(v)).replace("-", "m").replace("+", "")


F_EDITS = ([("corr.a", v) for v in (-1.0, -0.3, 0.0)] + [("conc.a", v) for v in (0.0, 500.0, -500.0)] +
           [("conc.b", v) for v in (800.0, -800.0)] + [("corr.b", -800.0)] + [("fail.r", -np.inf), ("fail.r", 800.0)] +
           [("corr.theta", v) for v in (1e-2, 1e3)])
N_EDITS = [("corr.theta", v) for v in (np.inf, 0.0, -1.0, np.nan, 5e-324)] + [("corr.b", 800.0), ("fail.r", np.nan)]
N_PRIOR_EDITS = [("corr.a", -0.3), ("corr.a", 0.0), ("conc.a", 0.0)]
W_THETAS = (1e-8, 1e-4, 1e5, 1e8, 1e15, 1.7e308)
GRID_SIZES = (1, 2, 8, 9, 63, 64, 65, 256, 257, 447, 448, 449)
#: cases with table rows that are flat by construction, so that such a row's mode is a matter of
#: rounding (decided rows are still compared; only the 90% share is not asked of these):
#:   conc.b = -800   cfp = 1 at every point: every column is the constant log(1 / G);
#:   conc.a = +-500  cfp is a step, exactly 1 on one side of mag = 0.0104: the count-0 rows (a
#:                   third of the genes) are constant over that side;
#:   vshape          the grid visits every magnitude but one twice: each row has its values in
#:                   equal pairs, the maximum included where it lies on the doubled stretch;
#:   G = 1           one point (is_flat).
FLAT_NAMES = {"conc.b=" + _fmt(-800.0), "conc.a=" + _fmt(500.0), "conc.a=" + _fmt(-500.0), "vshape"}


def group_f(sizes=(401, 61)):
    out = []
    for G in sizes:
        for col, v in F_EDITS:
            for cell in ((3, 0, 7) if col == "corr.a" else (3,)):
                out.append(Case("F", f"{col}={_fmt(v)}", G, col, v, cell))
        for kind in MAG_SHAPES:
            out.append(Case("F", kind, G, mag=kind))
    return out


def group_n(sizes=(401, 61)):
    out = []
    for G in sizes:
        for col, v in N_EDITS:
            out.append(Case("N", f"{col}={_fmt(v)}", G, col, v))
        out.append(Case("N", "corr.b=700,corr.a=2", G, "corr.b", 700.0, second=("corr.a", 2.0)))
        for col, v in N_PRIOR_EDITS:
            out.append(Case("N", f"prior-{col}={_fmt(v)}", G, col, v, mag="prior"))
    return out


def group_w(sizes=(401, 61)):
    return [Case("W", f"theta={_fmt(t)}", G, "corr.theta", t) for G in sizes for t in W_THETAS]


def grid_sizes():
    out = []
    for G in GRID_SIZES:
        out.append(Case("G", "plain", G))
        out.append(Case("G", "corr.a=" + _fmt(-0.3), G, "corr.a", -0.3))
    return out


def wide_counts():
    return [Case("F", "plain", 401, wide=True), Case("F", "corr.a=" + _fmt(-0.3), 401, "corr.a", -0.3, wide=True)]


def is_flat(case):
    return case.name in FLAT_NAMES or case.G == 1


def decided_rows(post):
    """Rows of a genes x grid table whose maximum exceeds the runner-up by more than twice the
    bar, 2 (RTOL |v| + ATOL): two tables within the bar of each other agree on their modes."""
    p = np.asarray(post, np.float64)
    if p.shape[1] < 2:
        return np.ones(p.shape[0], bool)
    s = np.sort(p, axis=1)
    v, r = s[:, -1], s[:, -2]
    with np.errstate(invalid="ignore"):
        return (v - r) > 2 * (RTOL * np.abs(v) + ATOL)


# ------------------------------------------------------------------ wide-model fuzz
FUZZ_SEEDS = tuple(range(2000, 2008))
FUZZ_KW = dict(n_randomizations=7, n_cores=2, length_out=400)


def fuzz_case(seed):
    """Models far outside the fitted fixtures' ranges, through scde.expression.difference."""
    rng = np.random.default_rng(seed)
    n1, n2 = int(rng.integers(2, 20)), int(rng.integers(2, 20))
    C = n1 + n2
    models = {
        "conc.b": rng.uniform(-40, 40, C),
        "conc.a": rng.uniform(0.01, 50, C),
        "fail.r": np.log(rng.uniform(1e-3, 50, C)),
        "corr.b": rng.uniform(-5, 8, C),
        "corr.a": rng.uniform(0.05, 5, C),
        "corr.theta": np.exp(rng.uniform(math.log(1e-2), math.log(1e3), C)),
    }
    N = int(rng.integers(1, 61))
    mu = np.exp(rng.normal(1.5, 1.8, (N, 1)))
    cnt = rng.negative_binomial(2.0, 2.0 / (2.0 + mu), size=(N, C))
    cnt[rng.uniform(size=(N, C)) < 0.55] = 0
    groups = np.array([0] * n1 + [1] * n2)
    rng.shuffle(groups)
    return models, np.ascontiguousarray(cnt.astype(np.int32)), groups
