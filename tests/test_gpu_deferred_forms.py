"""The deferred DE and PSO / CPSO generation kernels (csrc/sx_de_kernel.hpp: sx_de.hip, sx_de_chain.hip; csrc/sx_pso.hip), form
by form, on all seven objectives: every case of tests/_deferred_cases.py through every launch form its shape admits, against
`oracle.minimize` run on the device's own objective values (`stochopy_amd.factory.<name>(X)`: sx_eval).  A row's value is the
same bits in every kernel, so every comparison is exact: populations, fitness vectors, best rows, generation counts and
statuses.  What the table exercises is asserted on the oracle alone by tests/test_deferred_cases_host.py.

A mismatch says where the runs part: the first generation, the number of rows, the first element -- and whether the
candidates' values (funall) of that generation differ as well (then the proposal or the objective is off, else the
selection or the store)."""
import numpy as np
import pytest

import _deferred_cases as dc

pytestmark = pytest.mark.gpu

TAG = lambda c: c.tag  # noqa: E731


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def expect_stop(case, ref):
    if case.kind == "run":
        assert (ref.res.nit, ref.res.status) == (dc.GENS, -1)
    else:
        assert (ref.res.nit, ref.res.status) == (dc.STOP_GEN, 1 if case.kind == "stop1" else 0)


@pytest.mark.parametrize("case", dc.CASES, ids=TAG)
def test_two_kernel_path_matches_oracle(sa, case):
    """`minimize(..., callback=..., return_all=True)`: one generation kernel and one best / termination kernel per generation
    (DE: XM = 0), host draws where the case asks for them."""
    ref = dc.device_reference(case)
    expect_stop(case, ref)
    res, pops = dc.minimize_on_device(sa, case)
    for g, (X, want) in enumerate(zip(pops, ref.pops), start=1):
        if not np.array_equal(X, want):
            cand = "differ too" if not np.array_equal(res.funall[g - 1], ref.res.funall[g - 1]) else "are equal"
            pytest.fail("generation %d: %s; the candidates' values %s" % (g, dc.first_difference(X, want), cand))
    assert len(pops) == ref.res.nit
    assert (res.nit, res.nfev, res.status) == (ref.res.nit, ref.res.nfev, ref.res.status)
    assert np.array_equal(res.funall, ref.res.funall), dc.first_difference(res.funall, ref.res.funall)
    assert np.array_equal(res.xall, ref.res.xall)
    assert float(res.fun) == float(ref.res.fun) and np.array_equal(res.x, ref.res.x)


@pytest.mark.parametrize("case", dc.PHILOX_CASES, ids=TAG)
def test_stepwise_launches_match_oracle(case):
    """`_DeRun` (the chained kernel, XM = 1) / `_PsoRun` driven one `enqueue(1)` at a time: after every launch the population,
    the fitness vector, the best row and the state are the oracle's; the run stops where the oracle does, and a launch
    enqueued behind the stop changes no row, no fitness value and not the state."""
    from stochopy_amd import _lib

    ref = dc.device_reference(case)
    expect_stop(case, ref)
    run = dc.make_run(case)
    try:
        got, status, before, after = dc.stepwise(run, dc.GENS)
    finally:
        run.close()
    for g, (st, X, fit, best) in enumerate(got, start=1):
        assert int(st.it) == g
        if not np.array_equal(X, ref.pops_after[g - 1]):
            cand = "differs too" if not np.array_equal(fit, ref.fit_after[g - 1]) else "is equal"
            pytest.fail("generation %d: %s; the fitness vector %s" % (g, dc.first_difference(X, ref.pops_after[g - 1]), cand))
        assert np.array_equal(fit, ref.fit_after[g - 1]), "generation %d: %s" % (g, dc.first_difference(fit, ref.fit_after[g - 1]))
        assert int(st.gbidx) == int(np.argmin(ref.fit[g - 1])), g
        assert float(st.gfit) == ref.best_f[g - 1], g
        assert np.array_equal(best, ref.best_x[g - 1]), g
        assert bool(st.done) == (g == ref.res.nit), g
        if not st.done:
            assert int(st.status) == _lib.SX_STATUS_NONE
    assert len(got) == ref.res.nit and status == ref.res.status
    assert dc.same_snapshot(before, after), "a launch behind the stop wrote something"


@pytest.mark.parametrize("case", dc.GRAPH_CASES, ids=TAG)
def test_replayed_graphs_end_in_the_oracles_result(sa, case):
    """A whole `minimize()` of GRAPH_GENS generations with nothing watching: replayed graphs (DE: the tail chunk twice; PSO /
    CPSO: one chunk, with the restart carried into the next generation kernel), then eager launches."""
    ref = dc.device_reference(case, dc.GRAPH_GENS)
    assert (ref.res.nit, ref.res.status) == (dc.GRAPH_GENS, -1)
    assert not case.restart or len(ref.restarts) >= 1
    res, _ = dc.minimize_on_device(sa, case, dc.GRAPH_GENS, watch=False)
    assert (res.nit, res.status) == (ref.res.nit, ref.res.status)
    assert float(res.fun) == float(ref.res.fun)
    assert np.array_equal(res.x, ref.res.x), dc.first_difference(res.x[None, :], ref.res.x[None, :])
