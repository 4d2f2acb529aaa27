"""The conditions the tables of tests/_sample_edges.py rest on, checked on the numpy restatement alone (no GPU): a parity
case means something only if both outcomes of its decision occur, if no decision hangs on the last bits of a draw, and if the
reference it is compared with is itself good to well inside the bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_edges as edges  # noqa: E402

HMC_PROPOSALS = edges.HMC_CHAINS * (edges.HMC_MAXITER - 1)  # 72


@pytest.mark.parametrize("objective", edges.ALL)
def test_gradient_rows_have_a_reference_good_to_1e_13(objective):
    """Every row of the gradient table: the float64 closed form within 1e-13 of its norm of the np.longdouble evaluation
    (exactly equal where the gradient is identically zero), and the planted rows are what they are meant to be."""
    for n in edges.GRAD_NS:
        X, want = edges.gradient_rows(objective, n), edges.gradient_reference(objective, n)
        assert X.shape == want.shape == (edges.GRAD_ROWS, n) and np.all(np.abs(X) <= 5.0) and np.all(np.isfinite(want))
        exact = edges.gradient_longdouble(objective, X)
        err = np.linalg.norm((want - exact).astype(np.float64), axis=1)
        assert np.all(err <= edges.GRAD_REF_RTOL * np.linalg.norm(want, axis=1)), (n, err.max())
        lpr = edges.lanes_per_row(n)
        assert not X[0].any() and np.all(X[1] == 1.0) and np.all(X[3] == np.rint(X[3]))
        assert sorted(np.flatnonzero(X[2])) == sorted({e for e in (lpr - 1, lpr, n - 1) if e < n})
        if objective in ("ackley", "griewank", "quartic", "rastrigin", "sphere"):
            assert not want[0].any()
        if objective == "rosenbrock":
            assert not want[1].any()
            assert n > 1 or not want.any()
            if n > lpr:  # the 1.5 of element LPR reaches element LPR - 1 (the last lane) through its right neighbour
                assert want[2, lpr - 1] == -400.0 * 1.5 * (1.5 - 1.5**2) - 2.0 * (1.0 - 1.5) + 200.0 * 1.5
        if objective == "griewank":
            assert np.all(np.cos(X / np.sqrt(np.arange(1, n + 1))) != 0.0)


def test_hmc_cases_accept_and_reject():
    """Short hmc chains: the narrow starts of rosenbrock and quartic accept every proposal (from the whole box they would
    accept none from n = 17 on), and over the full-box cases the restatement rejects as well as accepts."""
    rejected = {}
    for case in edges.HMC_CASES:
        name, n, jac = case
        want = edges.hmc_reference(case)
        assert np.all(np.isfinite(want.funall)) and want.nit == edges.HMC_MAXITER
        assert want.nfev == edges.HMC_CHAINS * (1 + 3 * (0 if jac else 2 * n * (edges.HMC_NLEAP + 2))) + 2 * HMC_PROPOSALS
        if name in edges.HMC_NARROW:
            assert int(want.nacc.sum()) == HMC_PROPOSALS, case
            assert edges.hmc_x0(name, n).shape == (edges.HMC_CHAINS, n)
            assert np.array_equal(want.xall[:, 0], edges.hmc_x0(name, n))
        else:
            rejected[case] = HMC_PROPOSALS - int(want.nacc.sum())
    assert sum(rejected.values()) > 0
    for (name, n, jac), r in rejected.items():
        if name == "rastrigin" and n <= 33:
            assert 3 <= r <= 6, (name, n, jac, r)  # 66 to 69 of 72 accepted


def test_hmc_tolerances_come_from_the_committed_printout():
    """A case's x tolerance is 1000 times the deviation tools/sample_sensitivity.py --edges printed for it (at least 1e-12 of
    the range), and no case needs more than the project's 1e-6; no acceptance count moved under the perturbation."""
    printed = edges.hmc_sensitivity()
    assert sorted(printed) == sorted(edges.hmc_id(c) for c in edges.HMC_CASES)
    for case in edges.HMC_CASES:
        deviation, same_counts = printed[edges.hmc_id(case)]
        assert same_counts, case
        tol = edges.hmc_xtol(case)
        assert 1.0e-12 <= tol <= edges.PROJECT_XTOL
        assert tol == max(1.0e-12, 1000.0 * deviation) or (tol == edges.PROJECT_XTOL and case == ("rastrigin", 257, None))
        if case[2] == "analytic":
            assert deviation <= 1.1e-14


@pytest.mark.parametrize("case", edges.REJECT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_reject_cases_reject_through_the_planted_element(case):
    """Both outcomes of the feasibility test occur, every infeasible proposal is infeasible in the planted element alone, and
    no proposal's planted element comes within 1e-12 of the range of a bound (the decision does not hang on the last bits
    of a normal)."""
    method, n, e = case
    want, proposals = edges.reject_reference(case)
    feasible = int(want.nfeas.sum())
    assert 0 < feasible < edges.REJECT_TOTAL
    lo, hi = (63, 101) if method == "mcmc" else (77, 97)
    print(case, "feasible proposals", feasible, "of", edges.REJECT_TOTAL)
    assert lo <= feasible <= hi  # (the ranges seen when the table was chosen)
    assert proposals.shape == (edges.REJECT_MAXITER - 1, edges.REJECT_CHAINS, n)
    others = np.delete(proposals, e, axis=2)
    assert np.all(np.abs(others) < 0.5 * edges.UPPER)
    outside = (proposals[:, :, e] < edges.LOWER) | (proposals[:, :, e] > edges.UPPER)
    assert int(outside.sum()) == edges.REJECT_TOTAL - feasible
    distance = np.minimum(np.abs(proposals[:, :, e] - edges.LOWER), np.abs(proposals[:, :, e] - edges.UPPER))
    assert distance.min() > edges.REJECT_MARGIN * edges.SPAN
    assert np.all(want.xall >= edges.LOWER) and np.all(want.xall <= edges.UPPER)
    assert 0 < int(want.nacc.sum()) <= feasible


def test_mcmc_cases_cover_the_layout_edges():
    """Every objective and every n of the table occur, blocks of one variable included, and both outcomes of the decision
    occur over the table."""
    assert {c[0] for c in edges.MCMC_CASES} == set(edges.ALL)
    assert {c[1] for c in edges.MCMC_CASES} == set(edges.MCMC_NS)
    assert len({edges.mcmc_id(c) for c in edges.MCMC_CASES}) == len(edges.MCMC_CASES)
    accepted = total = 0
    for case in edges.MCMC_CASES:
        name, n, perc, chains = case
        want = edges.mcmc_reference(case)
        if perc * n <= 1.0 + 1e-9:
            assert max(1, int(perc * n)) == 1
        accepted += int(want.nacc.sum())
        total += chains * (edges.MCMC_MAXITER - 1)
    assert 0 < accepted < total
