"""options["runs"]: asking a batch for its optional outputs changes nothing else.  minimize(..., runs=3) binds none of them
(they stay NULL in the kernel's arguments); the same batch built with every one of them (each method's _runs_batch, which
minimize() itself calls) returns xs, funs, nits, statuses -- and sigmas -- bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P, MAXITER, SEED, R = 6, 8, 5, 3, 3
BOUNDS = [[-5.12, 5.12]] * N
# method -> module of optimize/, its arguments between (seeds, fun_id, lower, upper, x0, maxiter, P) and (xtol, ftol) at
# minimize()'s defaults, every optional output, further options of the call
POPULATION = {"rng": "philox", "updating": "deferred"}
CASES = {
    "de": ("_de", (0.5, 0.9, "best1bin", None), ("xfinal",), POPULATION),
    "pso": ("_cpso", (0.7298, 1.49618, 1.49618, None, None), ("xfinal", "pbest_final", "pbestfit_final"), POPULATION),
    "cpso": ("_cpso", (0.7298, 1.49618, 1.49618, 1.0, None), ("xfinal", "pbest_final", "pbestfit_final"), POPULATION),
    "cmaes": ("_cmaes", (0.1, 0.5), ("nfevs", "xmeans"), {"rng": "philox"}),
    "vdcma": ("_vdcma", (0.1, 0.5), ("nfevs", "xmeans", "dvecs", "vvecs"), {"rng": "philox"}),
}


@pytest.mark.parametrize("method", sorted(CASES))
def test_optional_outputs_change_nothing_else(method):
    import importlib

    import stochopy_amd as sa
    from stochopy_amd import _lib

    module, own, optional, more = CASES[method]
    res = sa.optimize.minimize(sa.factory.rosenbrock, BOUNDS, method=method,
                               options=dict(more, popsize=P, maxiter=MAXITER, seed=SEED, runs=R))
    lower, upper = np.full(N, -5.12), np.full(N, 5.12)
    build = importlib.import_module("stochopy_amd.optimize." + module)._runs_batch
    batch = build([SEED + r for r in range(R)], _lib.FUN_IDS["rosenbrock"], lower, upper, None, MAXITER, P, *own, 1.0e-8, 1.0e-8,
                  outputs=optional)
    batch.launch()
    out = batch.fetch()
    assert set(optional) <= set(out)
    shared = ["xs", "funs", "nits", "statuses"] + (["sigmas"] if method in ("cmaes", "vdcma") else [])
    assert (res.nits >= 1).all() and res.xs.shape == (R, N)
    for name in shared:
        assert res[name].dtype == out[name].dtype and res[name].tobytes() == out[name].tobytes(), name
