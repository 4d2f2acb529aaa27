"""The ordered sweeps of csrc/sx_async.hip (updating="immediate", what a plain de / pso / cpso call runs) on every objective,
row width and workgroup geometry, at ties of the `<=` rules and on a sweep that is one dependency chain -- whole runs with
in-kernel Philox draws against the oracle, and sx_de_async_generation through the C ABI against a plain loop.

The table and the ABI driver live in tests/_async_abi.py; tools/immediate_sensitivity.py shows on the oracle alone that no
decision of a table case hinges on the last bits of an objective value (profiles/immediate_edges_sensitivity.txt), which is
what lets positions be compared bit for bit where the objective itself is only good to 1e-13."""
import numpy as np
import pytest

import oracle
import _async_abi as abi

pytestmark = pytest.mark.gpu

EXACT = {"rosenbrock", "sphere"}  # + - * only: numpy's bits
RTOL_TRANSCENDENTAL = 1e-13       # the device's cos / exp / sqrt / pow against numpy's, as in test_objectives_vs_oracle
# Shrink with an objective outside EXACT: the oracle's own run moves by up to 1e-14 of the range when its objective values
# move by 2e-13 (a particle shrunk onto the boundary moves by a few ulp and its acceptance hangs on the last bits of f), so
# positions are held to 1000 times that; a wrong draw, lane or element moves one by >= 1e-3 of the range
SHRINK_XTOL_OF_RANGE, SHRINK_FUN_RTOL = 1e-11, 1e-9


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def _both(sa, method, objective, bounds, opts, x0=None):
    ref = oracle.minimize(objective, bounds, x0=None if x0 is None else x0.copy(), method=method, options=dict(opts), rng="philox")
    res = sa.optimize.minimize(getattr(sa.factory, objective), bounds, x0=x0, method=method,
                               options=dict(opts, backend="hip", rng="philox", strict_updating=True))
    return ref, res


@pytest.mark.parametrize("case", abi.EDGE_CASES, ids=abi.case_id)
def test_immediate_edges_vs_oracle(sa, case):
    """A tiny whole run per edge (one workgroup, <= 20 generations): nit / nfev / status equal; everything bit for bit for the
    + - * objectives; positions bit for bit and values within 1e-13 for the others; bounds for Shrink with those."""
    method, objective, bounds, opts = abi.case_options(case)
    ref, res = _both(sa, method, objective, bounds, opts)
    width = abi.RANGE[1] - abi.RANGE[0]
    assert res.xall.shape == ref["xall"].shape and res.funall.shape == ref["funall"].shape
    dx = float(np.abs(res.xall - ref["xall"]).max()) / width
    df = float((np.abs(res.funall - ref["funall"]) / np.abs(ref["funall"])).max())
    print(f"\n{abi.case_id(case)}: n = {len(bounds)}, nit {res.nit}, status {res.status}, max |dxall| / range = {dx:.3g}, "
          f"max rel dfunall = {df:.3g}, rel dfun = {abs(res.fun - ref['fun']) / abs(ref['fun']):.3g}")
    assert (res.nit, res.nfev, res.status) == (ref["nit"], ref["nfev"], ref["status"])
    if objective in EXACT:
        assert np.array_equal(res.x, ref["x"]) and res.fun == ref["fun"]
        assert np.array_equal(res.xall, ref["xall"]) and np.array_equal(res.funall, ref["funall"])
    elif opts.get("constraints") != "Shrink":
        assert np.array_equal(res.xall, ref["xall"]) and np.array_equal(res.x, ref["x"])
        assert np.allclose(res.funall, ref["funall"], rtol=RTOL_TRANSCENDENTAL, atol=1e-13)
        assert np.isclose(res.fun, ref["fun"], rtol=RTOL_TRANSCENDENTAL, atol=1e-13)
    else:
        assert dx <= SHRINK_XTOL_OF_RANGE
        assert np.allclose(res.x, ref["x"], rtol=0, atol=SHRINK_XTOL_OF_RANGE * width)
        assert np.allclose(res.funall, ref["funall"], rtol=SHRINK_FUN_RTOL, atol=0)
        assert np.isclose(res.fun, ref["fun"], rtol=SHRINK_FUN_RTOL, atol=0)


# ---------------------------------------------------------------------------------------------------------------------------
# Ties.  selection_async accepts on fc <= fold and improves the best on fc <= gfit: with equal rows every individual of a
# round is accepted AND an improver (dx = 0) -- the longest walk there is (best* strategies and PSO end a run after every
# improver) -- and only the last individual's status survives the sweep.
# ---------------------------------------------------------------------------------------------------------------------------
TIE_N, TIE_P = 5, 70
TIE_METHODS = [("de", {"strategy": "best1bin"}), ("de", {"strategy": "rand1bin"}), ("pso", {})]


def _tie_x0(kind):
    row = np.linspace(0.3, 1.1, TIE_N)
    if kind == "equal":
        return np.tile(row, (TIE_P, 1)), 4
    if kind == "zero":
        return np.zeros((TIE_P, TIE_N)), 4
    x0 = np.tile(row, (TIE_P, 1))  # "half": the walk alternates between tied and ordinary individuals
    x0[TIE_P // 2:] = np.random.RandomState(4).uniform(abi.RANGE[0], abi.RANGE[1], (TIE_P - TIE_P // 2, TIE_N))
    assert len(np.unique(x0[TIE_P // 2:], axis=0)) == TIE_P - TIE_P // 2
    return x0, 6


@pytest.mark.parametrize("kind", ["equal", "zero", "half"])
@pytest.mark.parametrize("method,extras", TIE_METHODS, ids=lambda v: v if isinstance(v, str) else v.get("strategy", ""))
def test_immediate_ties_vs_oracle(sa, method, extras, kind):
    """sphere, n = 5, P = 70 (a round of 64 and one of 6), a population of equal rows: the oracle's run, bit for bit.
    "equal": every trial ties its parent and the best, the run ends by maxiter (-1).  "zero": f = 0 <= ftol, every individual
    leaves status 0, the last one included: the run ends after its first sweep.  "half": 35 equal rows, then 35 distinct ones."""
    x0, maxiter = _tie_x0(kind)
    keep = x0.copy()
    bounds = [list(abi.RANGE)] * TIE_N
    opts = dict(extras, popsize=TIE_P, maxiter=maxiter, seed=abi.SEED, updating="immediate", return_all=True)
    ref, res = _both(sa, method, "sphere", bounds, opts, x0=x0)
    print(f"\nties {method} {extras.get('strategy', '')} {kind}: nit {res.nit} / {ref['nit']}, status {res.status} / {ref['status']}, "
          f"fun {res.fun!r} / {ref['fun']!r}, xall equal: {res.xall.shape == ref['xall'].shape and np.array_equal(res.xall, ref['xall'])}")
    assert (res.nit, res.nfev, res.status, res.success, res.message) == (
        ref["nit"], ref["nfev"], ref["status"], ref["success"], ref["message"])
    assert (ref["nit"], ref["status"]) == {"equal": (4, -1), "zero": (2, 0), "half": (6, -1)}[kind]  # (the oracle's, checked on the CPU)
    assert np.array_equal(res.x, ref["x"]) and res.fun == ref["fun"]
    assert np.array_equal(res.xall, ref["xall"]) and np.array_equal(res.funall, ref["funall"])
    if kind != "half":  # nothing ever moves
        assert np.array_equal(res.xall, np.broadcast_to(keep, res.xall.shape))
    if method == "pso":  # the caller's x0 is the working swarm (cpso/_cpso.py:389): it holds the last generation
        assert np.array_equal(x0, ref["xall"][-1])
        assert np.array_equal(x0, keep) == (kind != "half")


# ---------------------------------------------------------------------------------------------------------------------------
# One dependency chain: donor t of individual i is individual i - 1 - t and every element takes the mutant, so every
# individual of a round reads rows that the individuals right before it may just have replaced.
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 100, 300])  # 16 / 32 / 64 lanes per row: rounds of 64 / 32 / 16 individuals
@pytest.mark.parametrize("strategy", ["best1bin", "rand1bin"])
def test_de_sweep_of_chained_donors(strategy, n):
    """sx_de_async_generation on crafted host draws, P = 200, two generations, sphere on [2, 4]^n, F = 0.3, against the plain
    loop over i (oracle.engine.de_mutants + async_select): population, fit, candfit, best row and state, bit for bit."""
    P, generations = 200, 2
    inp = abi.chain_inputs(P, n, strategy)
    assert np.array_equal(inp["donors"][0], (np.arange(P) - 1) % P) and not inp["r1"].any()
    want = abi.chain_reference(inp, strategy, generations)
    # what makes the sweep a chain: more than half the trials replace their parents, so every round holds individuals whose
    # donor was replaced just before them (a property of the reference alone)
    assert all(w["accepted"] > P // 2 for w in want), [w["accepted"] for w in want]
    got = abi.chain_sweeps(inp, strategy, generations)
    print(f"\nchain {strategy} n = {n}: accepted per sweep {[w['accepted'] for w in want]}, state {[g['state'] for g in got]}")
    for g, w in zip(got, want):
        assert np.array_equal(g["candfit"], w["candfit"])
        assert np.array_equal(g["fit"], w["fit"])
        assert np.array_equal(g["X"], w["X"])
        assert np.array_equal(g["gbest"], w["gbest"])
        assert g["state"] == w["state"]
