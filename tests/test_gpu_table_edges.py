"""The posterior tables on the GPU (k_col_consts, k_tables_lpc with its tables_column_reg fallback,
the gated k_tables pass, k_tables above 448 points) at the model-parameter and grid-size edges of
tests/table_edge_cases.py, through logBootPosterior against the oracle's logBootPosterior with the
same arguments.

Per case: every cell's table with NaN, +inf and -inf exactly where the oracle has them and finite
values within rtol 1e-11 / atol 1e-13 (the bar of test_gpu_parity.test_logBootPosterior_esmef);
the joint posterior by assert_posterior_close; the modes where the oracle's row maximum is
decided; the other cells' tables bit-identical to the run with the edited cell restored (an odd
cell must not disturb the lean cells that share its launch); a repeated call with the same bits.
Group N (models whose tables the oracle fills with NaN) must be refused with an error that names
the model row and the column, before anything is launched.  Group W (theta outside the range the closed-form NB log-pmf was checked on) passes at the same
bar or, failing that, within 16 times the float64 oracle's own error against the 60-digit
restatement tests/tables_ref.py (the rule of tests/test_distance.py)."""
import sys

import numpy as np
import pytest

import table_edge_cases as E
import tables_ref as TR
from conftest import assert_cz_close, assert_posterior_close, assert_z_close

pytestmark = pytest.mark.gpu

MINLOGPROB = -sys.float_info.max / E.NCELLS / 1.1
MARGIN = 16.0
_ids = lambda cases: [c.id for c in cases]  # noqa: E731

# every context option these tests touch, with its default (include/scde_hip.h)
OPTION_DEFAULTS = {"boot_skip": 1, "boot_tiles": 1, "boot_tiles_cells": 400}
BOOT_PATHS = {"stretch": {}, "tiles": {"boot_tiles_cells": 0}, "stretch-forced": {"boot_tiles_cells": 0, "boot_tiles": 0},
              "noskip": {"boot_skip": 0}}


@pytest.fixture(scope="module")
def api():
    from scde_amd import api as A
    A.set_rand("glibc")
    return A


def run_gpu(api, case, restored=False, opts=None, ctx=None):
    """logBootPosterior on the default context of the Python layer (or ctx), under opts."""
    cx = ctx if ctx is not None else api.default_context()
    api.set_rand("glibc")
    for k, v in (opts or {}).items():
        cx.set_option(k, v)
    try:
        return api.logBootPosterior(*case.args(restored=restored), ctx=cx)
    finally:
        for k in (opts or {}):
            cx.set_option(k, OPTION_DEFAULTS[k])


_restored = {}


def gpu_restored(api, case):
    key = (case.G, case.mag_kind, case.wide)
    if key not in _restored:
        _restored[key] = run_gpu(api, case, restored=True)
    return _restored[key]


def same_bits(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def assert_same_call(a, b, what):
    assert same_bits(a["jp"], b["jp"]), f"{what}: jp differs"
    assert same_bits(a["modes"], b["modes"]), f"{what}: modes differ"
    for j, (p, q) in enumerate(zip(a["post"], b["post"])):
        assert same_bits(p, q), f"{what}: post of cell {j} differs"


def post_figures(got, ref):
    """(special positions equal, max |d| over finite entries, max ratio to the bar)."""
    same = (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == np.inf, ref == np.inf) and
            np.array_equal(got == -np.inf, ref == -np.inf))
    fin = np.isfinite(ref) & np.isfinite(got)
    if not fin.any():
        return same, 0.0, 0.0
    d = np.abs(got[fin] - ref[fin])
    return same, float(d.max()), float((d / (E.RTOL * np.abs(ref[fin]) + E.ATOL)).max())


def check_cell(got, ref, what):
    same, d, ratio = post_figures(got, ref)
    assert same, f"{what}: NaN / inf positions differ from the oracle's"
    assert ratio <= 1.0, f"{what}: max |gpu - oracle| {d:.3e}, {ratio:.3g} of the bar"


def check_modes(got, ref, cells, what):
    for j in cells:
        dec = E.decided_rows(ref["post"][j])
        np.testing.assert_array_equal(got["modes"][dec, j], ref["modes"][dec, j], err_msg=f"{what}: modes of cell {j}")


def check_case(api, oracle, case, skip_cell=None):
    """Everything asked of a case but the edited cell's table when skip_cell is set (group W)."""
    ref = oracle.logBootPosterior(*case.args())
    got = run_gpu(api, case)
    figs = [post_figures(got["post"][j], ref["post"][j]) for j in range(E.NCELLS)]
    print(f"{case.id}: max |gpu - oracle| per cell " + " ".join(f"{d:.1e}({r:.2g})" for _, d, r in figs) +
          f" (ratio to the bar in brackets); jp NaN share {np.isnan(got['jp']).mean():.2f} vs "
          f"{np.isnan(ref['jp']).mean():.2f}")
    cells = [j for j in range(E.NCELLS) if j != skip_cell]
    for j in cells:
        check_cell(got["post"][j], ref["post"][j], f"{case.id} cell {j}")
    if skip_cell is None:
        assert np.array_equal(np.isnan(got["jp"]), np.isnan(ref["jp"])), f"{case.id}: jp NaN positions"
        assert_posterior_close(got["jp"], ref["jp"], what=f"{case.id} jp")
    check_modes(got, ref, cells, case.id)
    if case.edited:
        rest = gpu_restored(api, case)
        for j in range(E.NCELLS):
            if j != case.cell:
                assert same_bits(got["post"][j], rest["post"][j]), \
                    f"{case.id}: cell {j}'s table changed with cell {case.cell}'s model"
    assert_same_call(run_gpu(api, case), got, f"{case.id} repeated")
    return got, ref


F_CASES = E.group_f()
N_CASES = E.group_n()
G_CASES = E.grid_sizes()
W_CASES = E.group_w()
WIDE_CASES = E.wide_counts()


@pytest.mark.parametrize("case", F_CASES, ids=_ids(F_CASES))
def test_group_f(api, oracle, case):
    check_case(api, oracle, case)


@pytest.mark.parametrize("case", N_CASES, ids=_ids(N_CASES))
def test_group_n(api, oracle, case):
    """Models whose tables the oracle fills with NaN (tests/test_table_edges.py test_oracle_nan) are
    refused before anything is launched, with a message that names the model row and the column
    (include/scde_hip.h, deviations); the context goes on working afterwards."""
    from scde_amd._lib import ScdeError
    with pytest.raises(ScdeError, match=rf"model row {case.cell}: .*{case.col.replace('.', '[.]')} = "
                                        if case.col != "fail.r" else rf"model row {case.cell}: fail[.]r is NaN"):
        run_gpu(api, case)
    key = (case.G, case.mag_kind, case.wide)
    if case.mag_kind is None:  # (on the prior's grid the restored models are fine)
        before = _restored.get(key)
        after = run_gpu(api, case, restored=True)
        if before is not None:
            assert_same_call(after, before, f"{case.id}: the restored call after the refusal")
        _restored[key] = after


@pytest.mark.parametrize("case", G_CASES, ids=_ids(G_CASES))
def test_grid_sizes(api, oracle, case):
    check_case(api, oracle, case)


@pytest.mark.parametrize("case", WIDE_CASES, ids=_ids(WIDE_CASES))
def test_wide_counts(api, oracle, case):
    check_case(api, oracle, case)


@pytest.mark.parametrize("case", [c for c in F_CASES if c.G == 401], ids=_ids([c for c in F_CASES if c.G == 401]))
def test_bootstrap_paths(api, oracle, case):
    """The three bound instantiations of the tables kernels (kBoundStretch: the default below 400
    cells; kBoundTiles; kBoundNone) and the bootstrap kernels behind them, on tables that hold
    -2.04e307 clamps: int-packed tile bounds and float stretch bounds.  Same bits from all four."""
    ref = oracle.logBootPosterior(*case.args())
    ctx = api.default_context()
    got = {}
    for name, opts in BOOT_PATHS.items():
        got[name] = run_gpu(api, case, opts=opts)
        assert ctx.stat("boot_path") == (1 if name == "tiles" else 0), (name, ctx.stat("boot_path"))
        assert_posterior_close(got[name]["jp"], ref["jp"], what=f"{case.id} {name} jp")
        for j in range(E.NCELLS):
            check_cell(got[name]["post"][j], ref["post"][j], f"{case.id} {name} cell {j}")
    for name in BOOT_PATHS:
        assert_same_call(got[name], got["stretch"], f"{case.id} {name} vs stretch")


@pytest.mark.parametrize("case", W_CASES, ids=_ids(W_CASES))
def test_group_w(api, oracle, case):
    """The edited cell's table: at the bar against the oracle, or within MARGIN x the oracle's own
    error of the exact column (every unique count at 61 points, 12 of them at 401).  Measured on
    an MI355X, max |gpu - exact| against the oracle's max |oracle - exact|: DESIGN.md section 4.0d."""
    got, ref = check_case(api, oracle, case, skip_cell=case.cell)
    c = case.cell
    same, d, ratio = post_figures(got["post"][c], ref["post"][c])
    mm, ucl, uci, mag = case.args()[:4]
    exact = TR.exact_rows(mm[c], ucl[c], uci[:, c], mag, ref["post"][c], MINLOGPROB, None if case.G <= 61 else 12)
    own, _ = TR.max_error(ref["post"][c], exact, E.RTOL, E.ATOL)
    err, over = TR.max_error(got["post"][c], exact, E.RTOL, E.ATOL, margin_abs=MARGIN * own)
    print(f"{case.id}: edited cell max |gpu - oracle| {d:.3e} ({ratio:.3g} of the bar); max |gpu - exact| {err:.3e}, "
          f"max |oracle - exact| {own:.3e}, {over:.3g} of {MARGIN:g} x own + bar")
    assert same, f"{case.id}: NaN / inf positions differ from the oracle's"
    if ratio > 1.0:  # (the oracle is then no reference for this cell's modes or for the joint posterior)
        assert over <= 1.0, f"{case.id}: |gpu - exact| {err:.3e} beyond {MARGIN:g} x {own:.3e} + bar"
        return
    assert_posterior_close(got["jp"], ref["jp"], what=f"{case.id} jp")
    check_modes(got, ref, [c], case.id)


def test_stale_slots_between_calls(api):
    """The table rows are reused between calls and k_tables_lpc leaves [ceil64(G), GS) unwritten:
    after a call that fills the rows up to 448 points (a cell of -2.04e307 clamps among them),
    shorter grids must give the bits a fresh context gives.  (NaN tables cannot be had: such models
    are refused, test_group_n.)"""
    filler = E.Case("F", "corr.a=-1", 448, "corr.a", -1.0)
    used = api.Context(0)
    try:
        got = run_gpu(api, filler, ctx=used)
        assert got["post"][filler.cell].min() == MINLOGPROB
        for G in (61, 330):
            plain = E.Case("B", "plain", G)
            fresh = api.Context(0)
            try:
                want = run_gpu(api, plain, ctx=fresh)
            finally:
                fresh.close()
            assert_same_call(run_gpu(api, plain, ctx=used), want, f"G = {G} after full rows at 448")
    finally:
        used.close()


@pytest.mark.parametrize("opts", [{}, {"boot_tiles_cells": 0}], ids=["default", "tiles"])
@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_wide_model_fuzz(api, oracle, seed, opts):
    from oracle import prior as OP
    models, counts, groups = E.fuzz_case(seed)
    kw = E.FUZZ_KW
    prior = OP.expression_prior(models, counts, kw["length_out"])
    ctx = api.default_context()
    api.set_rand("glibc")
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        got = api.scde_expression_difference(models, counts, {"x": prior["x"], "y": prior["y"]},
                                             groups=["a" if g == 0 else "b" for g in groups],
                                             n_randomizations=kw["n_randomizations"], n_cores=kw["n_cores"],
                                             return_posteriors=True)
    finally:
        for k in opts:
            ctx.set_option(k, OPTION_DEFAULTS[k])
    ref = oracle.scde_expression_difference(models, counts, prior["x"], prior["y"], groups,
                                            n_randomizations=kw["n_randomizations"], n_cores=kw["n_cores"],
                                            return_posteriors=True)
    for i in range(2):
        assert_posterior_close(got["joint.posteriors"][i], ref["joint.posteriors"][i], what=f"jp{i} seed {seed}")
    assert_posterior_close(got["difference.posterior"].values, ref["difference.posterior"], what=f"ratio seed {seed}")
    res = got["results"]
    for k in ("lb", "mle", "ub", "ce"):
        np.testing.assert_array_equal(res[k].to_numpy(), ref["results"][k], err_msg=f"{k} seed {seed}")
    assert_z_close(res["Z"].to_numpy(), ref["results"]["Z"], what=f"Z wide-model seed {seed}")
    assert_cz_close(res["cZ"].to_numpy(), ref["results"]["cZ"], res["Z"].to_numpy(), ref["results"]["Z"],
                    what=f"cZ wide-model seed {seed}")
