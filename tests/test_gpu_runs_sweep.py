"""options["runs"] = R with per-run hyperparameters (a sweep) on the GPU: `mutation`, `recombination`, `strategy` (de),
`inertia`, `cognitivity`, `sociability` (pso, cpso), `competitivity` (cpso), `sigma` (cmaes, vdcma) as sequences of R values,
through sx_*_runs_sweep_launch.  Run r is the single run with element r of every sequence and seed r: bit for bit for DE,
PSO and CPSO; for CMA-ES and VD-CMA bit for bit the run of the uniform batch with that sigma (the same kernel, the same
arithmetic, the same key: only where the scalar comes from differs) and, with the tolerances of
tests/test_gpu_cma_runs.py::_same_run, the single-run device loop and the numpy oracle.  A run depends on nothing but its own
seed and settings.  Every batch of this module is launched with its outputs filled with values no run produces, so an element
the kernel does not write cannot pass for a result."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from _runs_abi import FILL  # noqa: E402

pytestmark = pytest.mark.gpu

R = 16
STRATEGIES = ("rand1bin", "rand2bin", "best1bin", "best2bin")


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(autouse=True)
def filled_outputs(monkeypatch):
    """Every batch is launched over outputs that hold FILL (nits -7, statuses 77)."""
    from stochopy_amd.optimize import _runs

    launch = _runs.Batch.launch

    def filled(batch):
        with batch.stream():
            for name in batch.out:
                batch.dev[name].fill_({"nits": -7, "nfevs": -7, "statuses": 77}.get(name, FILL))
        launch(batch)

    monkeypatch.setattr(_runs.Batch, "launch", filled)


def _minimize(sa, method, obj, n, half, **opts):
    opts = dict(opts, backend="hip", rng="philox")
    if method in ("de", "pso", "cpso"):
        opts["updating"] = "deferred"
    return sa.optimize.minimize(getattr(sa.factory, obj), [[-half, half]] * n, method=method, options=opts)


def _written(res):
    assert not (res.xs == FILL).any() and not (res.funs == FILL).any()
    assert (res.nits > 0).all() and (res.statuses != 77).all()


def _bits(res, rows=slice(None)):
    parts = [res.xs[rows], res.funs[rows], res.nits[rows], res.statuses[rows]]
    if "sigmas" in res:
        parts.append(res.sigmas[rows])
    return tuple(np.ascontiguousarray(p).tobytes() for p in parts)


def _bitwise_single_runs(sa, method, obj, n, half, seeds, fixed, swept):
    """The sweep `swept` (option -> R values) over `seeds`, run r against the single call with element r of each."""
    got = _minimize(sa, method, obj, n, half, runs=len(seeds), seed=seeds, **fixed, **swept)
    _written(got)
    for r, seed in enumerate(seeds):
        own = {name: (values[r] if isinstance(values[r], str) else float(values[r])) for name, values in swept.items()}
        ref = _minimize(sa, method, obj, n, half, seed=int(seed), **fixed, **own)
        assert got.xs[r].tobytes() == np.asarray(ref.x).tobytes(), (r, own)
        assert float(got.funs[r]) == float(ref.fun) and int(got.nits[r]) == ref.nit and int(got.statuses[r]) == ref.status, (r, own)
    return got


# ---- 1. DE against single calls, bit for bit

FS, CRS = np.array([0.3, 0.5, 0.8, 1.2]), np.array([0.1, 0.5, 0.9, 1.0])
GRID = {"mutation": np.repeat(FS, 4), "recombination": np.tile(CRS, 4)}  # the 4 x 4 grid, R = 16
CYCLE = [STRATEGIES[(r + r // 4) % 4] for r in range(R)]                 # every strategy meets every F and every CR


@pytest.mark.parametrize("obj,n,P,strategy,constraints", [
    ("rosenbrock", 5, 8, CYCLE, None),
    ("rastrigin", 32, 32, CYCLE, None),
    ("sphere", 300, 6, "rand1bin", None),  # the row path above 256 elements
    ("rosenbrock", 5, 8, CYCLE, "Random"),
], ids=["n5-P8", "n32-P32", "n300-P6", "n5-P8-Random"])
def test_de_sweep_is_the_single_runs(sa, obj, n, P, strategy, constraints):
    fixed = {"popsize": P, "maxiter": 30 if n < 300 else 12, "constraints": constraints}
    swept = dict(GRID)
    if isinstance(strategy, str):
        fixed["strategy"] = strategy
    else:
        swept["strategy"] = strategy
        assert sorted(set(strategy)) == sorted(STRATEGIES)  # donor counts 2, 3, 4, 5 in one launch
    half = 1.0 if constraints else 5.12  # (Random: a narrow box, so mutants do leave it)
    _bitwise_single_runs(sa, "de", obj, n, half, [100 + 7 * r for r in range(R)], fixed, swept)


# ---- 2. PSO and CPSO against single calls, bit for bit

PSO_SWEEP = {"inertia": np.tile([0.4, 0.6, 0.7298, 0.9], 4), "cognitivity": np.repeat([0.5, 1.49618, 2.0, 3.0], 4),
             "sociability": np.tile([2.5, 1.49618, 1.0, 0.3], 4)[::-1].copy()}
GAMMAS = np.array([1.0, 0.0, 0.8, 1.2] * 4)  # one value 0: those runs never restart


@pytest.mark.parametrize("method,obj,n,P,half,maxiter,constraints", [
    ("pso", "rosenbrock", 5, 8, 5.12, 30, None),
    ("pso", "rastrigin", 32, 32, 5.12, 30, "Shrink"),
    ("cpso", "sphere", 5, 8, 0.5, 30, None),        # (a narrow box: the restarts of tests/test_gpu_pso_runs.py happen)
    ("cpso", "rastrigin", 32, 32, 0.5, 30, "Shrink"),
    ("pso", "sphere", 128, 64, 5.12, 10, None),     # the velocities live in the workspace
    ("cpso", "sphere", 128, 64, 0.5, 10, None),
], ids=["pso-n5-P8", "pso-n32-P32-shrink", "cpso-n5-P8", "cpso-n32-P32-shrink", "pso-workspace", "cpso-workspace"])
def test_pso_sweep_is_the_single_runs(sa, method, obj, n, P, half, maxiter, constraints):
    from stochopy_amd import _lib

    assert (_lib.lib().sx_pso_runs_workspace_bytes(R, P, n) > 0) == (n == 128)
    swept = dict(PSO_SWEEP)
    if method == "cpso":
        swept["competitivity"] = GAMMAS
    fixed = {"popsize": P, "maxiter": maxiter, "constraints": constraints}
    _bitwise_single_runs(sa, method, obj, n, half, [300 + 5 * r for r in range(R)], fixed, swept)


# ---- 3. CMA-ES and VD-CMA: run r of a sweep is run r of the uniform batch with sigma[r], bit for bit

SIGMAS = (0.15, 0.3, 0.6, 1.2)


@pytest.mark.parametrize("method,obj,n,P,maxiter", [
    ("cmaes", "sphere", 10, 65, 30), ("cmaes", "rosenbrock", 20, 48, 30),  # both solver widths
    ("vdcma", "sphere", 8, 12, 60), ("vdcma", "rosenbrock", 300, 10, 20),
], ids=["cmaes-n10-P65", "cmaes-n20-P48", "vdcma-n8-P12", "vdcma-n300-P10"])
def test_sigma_sweep_is_the_uniform_batches(sa, method, obj, n, P, maxiter):
    seeds = [900 + 3 * r for r in range(R)]
    sigma = np.array([SIGMAS[(r + r // 4) % 4] for r in range(R)])
    got = _minimize(sa, method, obj, n, 3.0, runs=R, seed=seeds, popsize=P, maxiter=maxiter, sigma=sigma)
    _written(got)
    assert not (got.sigmas == FILL).any()
    for s in SIGMAS:
        uniform = _minimize(sa, method, obj, n, 3.0, runs=R, seed=seeds, popsize=P, maxiter=maxiter, sigma=s)
        rows = np.flatnonzero(sigma == s)
        assert len(rows) == 4 and _bits(got, rows) == _bits(uniform, rows), s


# ---- 4. CMA-ES and VD-CMA against the single-run device loop and the oracle

SWEEP_SEEDS = [1244, 1245, 1246, 1247]
DIRECT = [("cmaes", "sphere", 10, 65, 30), ("cmaes", "rosenbrock", 2, 10, 100), ("vdcma", "sphere", 8, 12, 60)]


@functools.lru_cache(maxsize=None)
def _oracle(method, obj, n, P, maxiter, sigma, seed):
    """One oracle run; computed once, shared (read-only)."""
    opts = {"maxiter": maxiter, "popsize": P, "seed": seed, "sigma": sigma}
    if method == "cmaes":
        opts["eigh"] = "canonical"
    return oracle.minimize(obj, [[-3.0, 3.0]] * n, method=method, rng="philox", options=opts)


def _same_run(got, r, ref, P):
    """tests/test_gpu_cma_runs.py::_same_run: nit, nfev, status, success exact; fun rtol 1e-6; x rtol 1e-5 / atol 1e-7."""
    status = int(got.statuses[r])
    assert (int(got.nits[r]), int(got.nits[r]) * P, status, status >= 0) == (ref.nit, ref.nfev, ref.status, ref.success), r
    assert np.isclose(got.funs[r], ref.fun, rtol=1e-6, atol=1e-300), (r, got.funs[r], ref.fun)
    assert np.allclose(got.xs[r], ref.x, rtol=1e-5, atol=1e-7), (r, got.xs[r], ref.x)


@pytest.mark.parametrize("method,obj,n,P,maxiter", DIRECT, ids=["cmaes-sphere-n10-P65", "cmaes-rosenbrock-n2-P10", "vdcma-sphere-n8-P12"])
def test_sigma_sweep_against_the_single_run_and_the_oracle(sa, method, obj, n, P, maxiter):
    sigma, seeds = np.repeat(SIGMAS, 4), SWEEP_SEEDS * 4
    got = _minimize(sa, method, obj, n, 3.0, runs=R, seed=seeds, popsize=P, maxiter=maxiter, sigma=sigma)
    _written(got)
    refs = [_oracle(method, obj, n, P, maxiter, float(sigma[r]), seeds[r]) for r in range(R)]
    print(method, obj, "nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    print("  oracle nit", [ref.nit for ref in refs], "status", [ref.status for ref in refs])
    print("  rel fun vs oracle", ["%.3g" % (abs(got.funs[r] - ref.fun) / max(abs(ref.fun), 1e-300)) for r, ref in enumerate(refs)])
    for r, ref in enumerate(refs):
        _same_run(got, r, ref, P)
    for r in range(R):
        single = _minimize(sa, method, obj, n, 3.0, seed=seeds[r], popsize=P, maxiter=maxiter, sigma=float(sigma[r]))
        _same_run(got, r, single, P)
    if obj == "rosenbrock":  # the runs stop on their own, at different generations, with status 1 or -1
        assert set(int(v) for v in got.statuses) == {1, -1} and len(set(int(v) for v in got.nits)) > 4


# ---- 5. independence, the NULL path, R = 2

# method -> (objective, n, half-width, fixed options, the sweep)
ANY = {
    "de": ("rosenbrock", 5, 5.12, {"popsize": 8, "maxiter": 20}, dict(GRID, strategy=CYCLE)),
    "pso": ("rosenbrock", 5, 5.12, {"popsize": 8, "maxiter": 20}, PSO_SWEEP),
    "cpso": ("sphere", 5, 0.5, {"popsize": 8, "maxiter": 30}, dict(PSO_SWEEP, competitivity=GAMMAS)),
    "cmaes": ("rosenbrock", 6, 3.0, {"popsize": 12, "maxiter": 30}, {"sigma": np.tile(SIGMAS, 4)}),
    "vdcma": ("rosenbrock", 8, 3.0, {"popsize": 12, "maxiter": 30}, {"sigma": np.tile(SIGMAS, 4)}),
}


@pytest.mark.parametrize("method", sorted(ANY))
def test_permuting_the_runs_permutes_the_outputs(sa, method):
    obj, n, half, fixed, swept = ANY[method]
    seeds = np.array([40 + 11 * r for r in range(R)])
    perm = np.random.RandomState(8).permutation(R)
    assert (perm != np.arange(R)).sum() > R // 2
    whole = _minimize(sa, method, obj, n, half, runs=R, seed=list(seeds), **fixed, **swept)
    moved = _minimize(sa, method, obj, n, half, runs=R, seed=list(seeds[perm]), **fixed,
                      **{name: np.asarray(values)[perm] for name, values in swept.items()})
    _written(whole)
    assert _bits(moved) == _bits(whole, perm)


@pytest.mark.parametrize("method", sorted(ANY))
def test_a_sweep_that_repeats_the_scalar_is_the_scalar_call(sa, method):
    """The arrays' path against the NULL path of the same kernel; and R = 2."""
    obj, n, half, fixed, swept = ANY[method]
    for runs in (R, 2):
        scalars = {name: values[2] for name, values in swept.items()}
        plain = _minimize(sa, method, obj, n, half, runs=runs, seed=60, **fixed, **scalars)
        swept_same = _minimize(sa, method, obj, n, half, runs=runs, seed=60, **fixed,
                               **{name: [value] * runs for name, value in scalars.items()})
        _written(plain)
        assert _bits(plain) == _bits(swept_same)
        assert "sweep" not in plain and sorted(swept_same.sweep) == sorted(swept)
    two = _minimize(sa, method, obj, n, half, runs=2, seed=[40 + 11 * 3, 40 + 11 * 9], **fixed,
                    **{name: [values[3], values[9]] for name, values in swept.items()})
    whole = _minimize(sa, method, obj, n, half, runs=R, seed=[40 + 11 * r for r in range(R)], **fixed, **swept)
    assert _bits(two) == _bits(whole, [3, 9])


# ---- 6. the result


@pytest.mark.parametrize("method", sorted(ANY))
def test_the_result_holds_the_sweep_and_describes_the_best_run(sa, method):
    obj, n, half, fixed, swept = ANY[method]
    given = {name: (list(values) if k % 2 else np.array(values)) for k, (name, values) in enumerate(swept.items())}
    first = next(iter(swept))
    res = _minimize(sa, method, obj, n, half, runs=R, seed=5, **fixed, **given)
    assert sorted(res.sweep) == sorted(swept)
    for name, values in swept.items():
        assert res.sweep[name].shape == (R,) and list(res.sweep[name]) == list(values), name
        assert res.sweep[name].dtype == (np.float64 if name != "strategy" else res.sweep[name].dtype)
    best = int(np.argmin(res.funs))
    assert res.run == best and (res.x == res.xs[best]).all() and res.fun == res.funs[best]
    assert res.nit == res.nits[best] and res.status == res.statuses[best]
    # only what was given as a sequence is listed
    one = _minimize(sa, method, obj, n, half, runs=R, seed=5, **fixed,
                    **{name: (values if name == first else values[0]) for name, values in swept.items()})
    assert list(one.sweep) == [first]


# ---- 7. the C ABI's own guard: a strategy element the launch could not read


def test_a_strategy_element_out_of_range_ends_its_run_alone(sa):
    """sx_de_runs_sweep_launch cannot read its device arrays: a strategy outside 0 .. 3, or one that draws more donors than
    popsize - 1, ends that run at entry (funs NaN, nits 0, statuses SX_STATUS_NONE = 100, xs untouched); its neighbours are
    the runs they always were.  (minimize() refuses both before the device is touched.)"""
    from stochopy_amd import _lib
    from stochopy_amd.optimize._de import _runs_batch

    n, P, seeds = 5, 4, [21, 22, 23, 24]
    lower, upper = np.full(n, -5.12), np.full(n, 5.12)
    names = np.array(["rand1bin", "best1bin", "rand1bin", "best1bin"])

    def launch(ids):
        batch = _runs_batch(seeds, _lib.FUN_IDS["rosenbrock"], lower, upper, None, 15, P, np.array([0.4, 0.5, 0.6, 0.7]), 0.9,
                            names, None, 1e-8, 1e-8)
        if ids is not None:
            with batch.stream():
                batch.sweep["strategy"].copy_(batch.ctx.upload_async(np.array(ids, dtype=np.int32)))
        batch.launch()  # (filled_outputs: over FILL)
        return batch.fetch()

    good = launch(None)
    assert (good["nits"] > 0).all() and not (good["xs"] == FILL).any()
    bad = launch([0, 7, 1, -1])  # 7 and -1: no strategy; 1 = rand2bin: five donors out of three other rows
    assert bad["xs"][0].tobytes() == good["xs"][0].tobytes() and bad["funs"][0] == good["funs"][0]
    assert bad["nits"][0] == good["nits"][0] and bad["statuses"][0] == good["statuses"][0]
    for r in (1, 2, 3):
        assert np.isnan(bad["funs"][r]) and bad["nits"][r] == 0 and bad["statuses"][r] == 100
        assert (bad["xs"][r] == FILL).all()
