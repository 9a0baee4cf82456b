"""The oracle on the posterior-table edge cases of tests/table_edge_cases.py (no GPU): the NaN /
finiteness pattern each group is built for, that one odd cell leaves the other cells' tables
untouched, that the rows' modes are decided where the GPU test compares them, and the 60-digit
restatement tests/tables_ref.py pinned against the oracle before it is used as an arbiter for
theta outside the fitted range (group W), where the float64 oracle's own error is what the
bound is made of."""
import sys

import numpy as np
import pytest

import table_edge_cases as E
import tables_ref as TR

F_CASES = E.group_f() + E.wide_counts()
N_CASES = E.group_n()
G_CASES = E.grid_sizes()
W_CASES = E.group_w()
_ids = lambda cases: [c.id for c in cases]  # noqa: E731
MINLOGPROB = -sys.float_info.max / E.NCELLS / 1.1

_restored = {}


def run(oracle, case, restored=False):
    if restored:  # the same call for every case on the same grid and counts: once
        key = (case.G, case.mag_kind, case.wide)
        if key not in _restored:
            _restored[key] = oracle.logBootPosterior(*case.args(restored=True))
        return _restored[key]
    return oracle.logBootPosterior(*case.args())


def check_others_untouched(oracle, case, ref):
    if not case.edited:
        return
    rest = run(oracle, case, restored=True)
    for j in range(E.NCELLS):
        if j != case.cell:
            assert np.array_equal(ref["post"][j], rest["post"][j]), f"{case.id}: cell {j} changed with cell {case.cell}"


@pytest.mark.parametrize("case", F_CASES + G_CASES + W_CASES, ids=_ids(F_CASES + G_CASES + W_CASES))
def test_oracle_finite(oracle, case):
    ref = run(oracle, case)
    for j, p in enumerate(ref["post"]):
        assert np.all(np.isfinite(p)), f"{case.id}: cell {j}"
        assert p.min() >= MINLOGPROB
    assert np.all(np.isfinite(ref["jp"]))
    rowsum = np.abs(ref["jp"].sum(1) - 1).max()
    assert rowsum <= 2e-15, rowsum
    check_others_untouched(oracle, case, ref)
    dec = E.decided_rows(ref["post"][case.cell])
    print(f"{case.id}: decided rows {dec.mean():.3f}, jp row sums within {rowsum:.1e}")
    if not E.is_flat(case):
        assert dec.mean() >= 0.9, f"{case.id}: only {dec.mean():.3f} of the rows have a decided mode"


@pytest.mark.parametrize("case", N_CASES, ids=_ids(N_CASES))
def test_oracle_nan(oracle, case):
    ref = run(oracle, case)
    assert np.all(np.isnan(ref["post"][case.cell])), case.id
    assert np.all(np.isnan(ref["jp"])), case.id
    for j in range(E.NCELLS):
        if j != case.cell:
            assert np.all(np.isfinite(ref["post"][j])), (case.id, j)
    check_others_untouched(oracle, case, ref)


@pytest.mark.parametrize("seed", E.FUZZ_SEEDS)
def test_oracle_fuzz_finite(oracle, seed):
    from oracle import prior as OP
    models, counts, groups = E.fuzz_case(seed)
    prior = OP.expression_prior(models, counts, E.FUZZ_KW["length_out"])
    ref = oracle.scde_expression_difference(models, counts, prior["x"], prior["y"], groups,
                                            n_randomizations=E.FUZZ_KW["n_randomizations"],
                                            n_cores=E.FUZZ_KW["n_cores"], return_posteriors=True)
    for jp in ref["joint.posteriors"]:
        assert not np.any(np.isnan(jp))
    z = ref["results"]["Z"]
    assert not np.any(np.isnan(z)) and np.abs(z).max() <= 7.17, z


def own_error(case, ref, ncols=12):
    """max |oracle - exact| over `ncols` exact columns of the edited cell, and its ratio to the bar."""
    mm, ucl, uci, mag = case.args()[:4]
    c = case.cell
    exact = TR.exact_rows(mm[c], ucl[c], uci[:, c], mag, ref["post"][c], MINLOGPROB, ncols)
    return TR.max_error(ref["post"][c], exact, E.RTOL, E.ATOL)


@pytest.mark.parametrize("G", [401, 61])
@pytest.mark.parametrize("cell", [0, 3, 7])
def test_restatement_meets_the_bar_on_the_base_case(oracle, G, cell):
    case = E.Case("B", "plain", G, cell=cell)
    ref = run(oracle, case)
    worst, ratio = own_error(case, ref)
    print(f"{case.id}: max |oracle - exact| {worst:.3e}, {ratio:.3g} of the bar")
    assert ratio <= 1.0, (worst, ratio)


@pytest.mark.parametrize("case", W_CASES, ids=_ids(W_CASES))
def test_oracle_own_error_wide_theta(oracle, case):
    """Reported, not bounded: the float64 oracle's own error against the exact column (p = theta /
    (theta + mu) rounds to 1 - O(eps) for large theta, and exp underflows where the exact value
    is still far above minlogprob).  Measured at 401 points: 9.4e-14 (theta 1e-8), 9.2e-14
    (1e-4), 2.9e-1 (1e5), 1.9e-2 (1e8), 1.0e1 (1e15), 2.2e3 (1.7e308)."""
    ref = run(oracle, case)
    worst, ratio = own_error(case, ref)
    print(f"{case.id}: max |oracle - exact| {worst:.3e}, {ratio:.3g} of the bar")
    assert np.isfinite(worst)
