"""options["runs"] = R around a caller's row-wise device objective, factory.batched(f, rowwise=True), on the GPU
(csrc/sx_runs_unfused.hip: R populations in device memory, one propose / move kernel for all R * P rows, ONE call of the
objective per generation, one selection kernel, one best / termination workgroup per run).  Run r of the batch is the single
run ``minimize(factory.batched(f), ..., seed=seed_r, rng="philox", updating="deferred")`` bit for bit -- and, where the shape
fits the LDS, run r of the resident factory batch --; runs stop on their own and stay frozen; the objective sees the stacked
``(R * P, n)`` tensor and nothing else."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def _bounds(n, half=5.12):
    return [[-half, half]] * n


@functools.lru_cache(maxsize=None)
def device_fun(name):
    """A "user" objective that happens to return the fused kernels' values, whatever the number of rows: sx_eval on the
    stream it is called on (tests/test_gpu_sample_batched.py device_objective)."""
    import torch

    from stochopy_amd import _lib

    L, fid = _lib.lib(), _lib.FUN_IDS[name]

    def fun(X):
        P, n = X.shape
        f = torch.empty((P,), dtype=torch.float64, device=X.device)
        X = X.contiguous()
        assert L.sx_eval(fid, X.data_ptr(), P, n, n, None, None, f.data_ptr(), None, None,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        return f

    fun.__name__ = "device_" + name
    return fun


@functools.lru_cache(maxsize=None)
def nonfinite_fun(name):
    """sx_eval's values, turned into NaN, +inf and exact ties by rules on the row's own content."""
    import torch

    inner = device_fun(name)

    def fun(X):
        f = torch.floor(inner(X))  # whole numbers: exact ties happen
        f = torch.where(X[:, 0] > 3.0, torch.full_like(f, float("nan")), f)
        f = torch.where(X[:, 1] < -3.0, torch.full_like(f, float("inf")), f)
        return f

    fun.__name__ = "nonfinite_" + name
    return fun


def weighted_quadratic(X, w, shift):
    """A user's own torch objective with args, accumulated column by column: element-wise operations only, so the value of a
    row cannot depend on how many rows there are."""
    import torch

    acc = torch.zeros(X.shape[0], dtype=X.dtype, device=X.device)
    for j in range(X.shape[1]):
        d = X[:, j] - shift
        acc = acc + w[j] * (d * d)
    return acc


def _rows32():
    from stochopy_amd import _lib

    return int(_lib.lib().sx_rows_per_workgroup(32))


def _x0(kind, R, P, n):
    if kind is None:
        return None
    rs = np.random.RandomState(5)
    return rs.uniform(-5.12, 5.12, (P, n) if kind == "shared" else (R, P, n))


SHRINK = {"constraints": "Shrink", "inertia": 1.0, "cognitivity": 3.0, "sociability": 3.0}  # particles do leave the box
RANDOM = {"constraints": "Random", "mutation": 1.5}                                          # repairs happen

# tag: (method, objective, n, popsize (or an offset to sx_rows_per_workgroup(32)), runs, seed, x0 kind, options)
CASES = {
    # fewer elements than lanes, best1bin's smallest population
    "de-n3-P4": ("de", "rosenbrock", 3, 4, 2, 7, None, {"maxiter": 12, "strategy": "best1bin"}),
    "pso-n3-P4": ("pso", "rosenbrock", 3, 4, 2, 7, None, {"maxiter": 12}),
    # the 16 -> 32 lanes-per-row boundary
    "de-n64-P16": ("de", "rosenbrock", 64, 16, 3, 21, None, {"maxiter": 10, "strategy": "rand1bin"}),
    "pso-n64-P16": ("pso", "rosenbrock", 64, 16, 3, 21, None, {"maxiter": 10}),
    "de-n65-P17": ("de", "rosenbrock", 65, 17, 3, 3, None, {"maxiter": 10, "strategy": "best1bin"}),
    "pso-n65-P17": ("pso", "rastrigin", 65, 17, 3, 3, None, {"maxiter": 10}),
    # whole-wave rows with a ragged last row step, rand2bin's smallest population
    "de-n130-P6": ("de", "rastrigin", 130, 6, 3, 8, None, {"maxiter": 10, "strategy": "rand2bin"}),
    "pso-n130-P6": ("pso", "rastrigin", 130, 6, 3, 8, None, {"maxiter": 10}),
    "de-n300-P16": ("de", "rosenbrock", 300, 16, 2, 2, None, {"maxiter": 8, "strategy": "best2bin"}),
    "pso-n300-P16": ("pso", "ackley", 300, 16, 2, 2, None, {"maxiter": 8}),
    # a ragged last workgroup of one run next to the first workgroup of the next run
    "de-rows-1": ("de", "ackley", 32, -1, 3, 9, None, {"maxiter": 10, "strategy": "best1bin"}),
    "de-rows": ("de", "ackley", 32, 0, 3, 9, None, {"maxiter": 10, "strategy": "best1bin"}),
    "de-rows+1": ("de", "ackley", 32, 1, 3, 9, None, {"maxiter": 10, "strategy": "best1bin"}),
    "pso-rows-1": ("pso", "ackley", 32, -1, 3, 9, None, {"maxiter": 10}),
    "pso-rows": ("pso", "ackley", 32, 0, 3, 9, None, {"maxiter": 10}),
    "pso-rows+1": ("pso", "ackley", 32, 1, 3, 9, None, {"maxiter": 10}),
    # more runs than the device has CUs
    "de-R300": ("de", "sphere", 3, 4, 300, 1000, None, {"maxiter": 6, "strategy": "best1bin"}),
    "pso-R300": ("pso", "sphere", 3, 4, 300, 1000, None, {"maxiter": 6}),
    # maxiter <= 1 still runs one generation; two generations
    "de-maxiter1": ("de", "rosenbrock", 10, 16, 3, 17, None, {"maxiter": 1}),
    "de-maxiter2": ("de", "sphere", 65, 6, 2, 18, None, {"maxiter": 2, "strategy": "rand2bin"}),
    "pso-maxiter1": ("pso", "rosenbrock", 10, 16, 3, 17, None, {"maxiter": 1}),
    "pso-maxiter2": ("pso", "sphere", 65, 6, 2, 18, None, {"maxiter": 2}),
    # unrelated seeds, one of them beyond 32 bits (both key words)
    "de-seed-sequence": ("de", "rosenbrock", 32, 32, 3, (977, 3, (1 << 40) + 17), None, {"maxiter": 20}),
    "pso-seed-sequence": ("pso", "rosenbrock", 32, 32, 3, (977, 3, (1 << 40) + 17), None, {"maxiter": 20}),
    "de-x0-shared": ("de", "sphere", 8, 16, 3, 19, "shared", {"maxiter": 12}),
    "de-x0-per-run": ("de", "rosenbrock", 130, 17, 2, 20, "per-run", {"maxiter": 8, "strategy": "rand1bin"}),
    "pso-x0-shared": ("pso", "sphere", 8, 16, 3, 19, "shared", {"maxiter": 12}),
    "pso-x0-per-run": ("pso", "rosenbrock", 130, 17, 2, 20, "per-run", {"maxiter": 8}),
    # repairs / scaled velocities
    "de-random-rand2bin": ("de", "sphere", 70, 33, 3, 13, None, dict(RANDOM, maxiter=10, strategy="rand2bin")),
    "de-random-best2bin": ("de", "rastrigin", 24, 40, 2, 16, None, dict(RANDOM, maxiter=10, strategy="best2bin")),
    "pso-shrink-n24": ("pso", "rastrigin", 24, 40, 2, 16, None, dict(SHRINK, maxiter=12)),
    "pso-shrink-n130": ("pso", "sphere", 130, 17, 3, 13, None, dict(SHRINK, maxiter=10)),
    "cpso-gamma0": ("cpso", "rosenbrock", 10, 20, 3, 31, None, {"maxiter": 12, "competitivity": 0}),
    # the STOP shape of tests/test_gpu_de_runs.py: runs end at different generations
    "de-stop": ("de", "sphere", 4, 32, 64, 13, None, {"maxiter": 400, "ftol": 1e-6, "xtol": 1e-3}),
    "pso-stop": ("pso", "sphere", 4, 32, 64, 13, None, {"maxiter": 400, "ftol": 1e-6, "xtol": 1e-3}),
    # beyond the LDS: the resident path refuses this population
    "de-beyond-lds": ("de", "rosenbrock", 128, 4096, 2, 23, None, {"maxiter": 3, "strategy": "rand1bin"}),
    "pso-beyond-lds": ("pso", "rosenbrock", 128, 4096, 2, 23, None, {"maxiter": 3}),
    # NaN, +inf and exact ties: the start kernel's argmin rules and the selection
    "de-nonfinite": ("de", "nonfinite:sphere", 6, 24, 4, 41, None, {"maxiter": 10, "strategy": "rand1bin"}),
    "pso-nonfinite": ("pso", "nonfinite:sphere", 6, 24, 4, 41, None, {"maxiter": 10}),
}
STOPPERS = ("de-stop", "pso-stop")
SLOW_SINGLES = STOPPERS + ("de-beyond-lds", "pso-beyond-lds", "de-nonfinite", "pso-nonfinite")


def _case(tag):
    method, objective, n, P, R, seed, x0kind, opts = CASES[tag]
    if "-rows" in tag:
        P = _rows32() + P
    return method, objective, n, P, R, seed, x0kind, opts


def _fun(objective):
    return nonfinite_fun(objective.split(":")[1]) if objective.startswith("nonfinite:") else device_fun(objective)


def _seeds(seed, R):
    return list(seed) if isinstance(seed, tuple) else [seed + r for r in range(R)]


@functools.lru_cache(maxsize=None)
def rowwise(tag, runs=None, **changes):
    import stochopy_amd as sa

    method, objective, n, P, R, seed, x0kind, opts = _case(tag)
    R = runs or R
    o = dict(opts, popsize=P, seed=list(seed) if isinstance(seed, tuple) else seed, rng="philox", updating="deferred",
             backend="hip", runs=R, **changes)
    x0 = _x0(x0kind, R, P, n)
    keep = None if x0 is None else x0.copy()
    res = sa.optimize.minimize(sa.factory.batched(_fun(objective), rowwise=True), _bounds(n), x0=x0, method=method, options=o)
    assert keep is None or np.array_equal(x0, keep)  # x0 is not modified
    return res


@functools.lru_cache(maxsize=None)
def single(tag, r, **changes):
    """Run r of the case through the single-run path: one minimize(factory.batched(f)) call of its own."""
    import stochopy_amd as sa

    method, objective, n, P, R, seed, x0kind, opts = _case(tag)
    s = seed[r] if isinstance(seed, tuple) else seed + r
    o = dict(opts, popsize=P, seed=s, rng="philox", updating="deferred", backend="hip", **changes)
    x0 = _x0(x0kind, R, P, n)
    if x0 is not None:
        x0 = (x0 if x0kind == "shared" else x0[r]).copy()  # (a single run works in place on x0)
    return sa.optimize.minimize(sa.factory.batched(_fun(objective)), _bounds(n), x0=x0, method=method, options=o)


def check_runs(got, singles, P):
    """tests/test_gpu_de_runs.py check_runs, NaN-aware (a NaN best value equals a NaN best value)."""
    R = len(singles)
    assert got.xs.shape == (R, len(singles[0].x)) and got.funs.shape == got.nits.shape == got.statuses.shape == (R,)
    for r, one in enumerate(singles):
        assert np.array_equal(got.xs[r], one.x), f"run {r}: x"
        assert np.array_equal(got.funs[r], one.fun, equal_nan=True), f"run {r}: fun {got.funs[r]!r} != {one.fun!r}"
        assert got.nits[r] == one.nit and got.statuses[r] == one.status, \
            f"run {r}: nit / status {got.nits[r]}, {got.statuses[r]} != {one.nit}, {one.status}"
    b = int(np.argmin(got.funs))
    assert got.run == b and np.array_equal(got.x, got.xs[b]) and np.array_equal(got.fun, got.funs[b], equal_nan=True)
    assert got.nit == got.nits[b] and got.status == got.statuses[b] and got.success == (got.status >= 0)
    assert got.message == singles[b].message
    assert got.nfev == int(got.nits.sum()) * P


# ---- 1. run r is the single run, bit for bit
@pytest.mark.parametrize("tag", sorted(set(CASES) - set(SLOW_SINGLES)))
def test_run_r_is_the_single_run_bit_for_bit(sa, tag):
    _, _, _, P, R, _, _, _ = _case(tag)
    check_runs(rowwise(tag), [single(tag, r) for r in range(R)], P)


CONSTRAINED = ("de-random-rand2bin", "de-random-best2bin", "pso-shrink-n24", "pso-shrink-n130")


@pytest.mark.parametrize("tag", CONSTRAINED)
def test_the_constraint_does_act(sa, tag):
    """Random does repair elements and Shrink does scale velocities in these cases: without the constraint every run ends
    elsewhere (the initial populations lie inside the box whatever its size, so what drives rows out of it is the
    coefficients, not the width of the bounds)."""
    _, _, _, _, R, _, _, _ = _case(tag)
    got, free = rowwise(tag), rowwise(tag, constraints=None)
    assert np.array_equal(got.nits, free.nits)
    for r in range(R):
        assert not np.array_equal(got.xs[r], free.xs[r]), f"run {r} never left the box"
    assert (np.abs(got.xs) <= 5.12 * (1 + 1e-12)).all()  # (Shrink lands on a bound to rounding)


def test_an_all_zero_competitivity_sequence_is_reported_as_on_the_resident_path(sa):
    method, objective, n, P, R, seed, _, opts = _case("cpso-gamma0")
    got = rowwise("cpso-gamma0", competitivity=(0.0,) * R)
    ref = sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n), method=method,
                               options=dict(opts, popsize=P, seed=seed, rng="philox", updating="deferred", runs=R,
                                            competitivity=[0.0] * R))
    assert sorted(got.sweep) == sorted(ref.sweep) == ["competitivity"]
    assert np.array_equal(got.sweep["competitivity"], ref.sweep["competitivity"])
    for key in ("xs", "funs", "nits", "statuses"):
        assert np.array_equal(got[key], ref[key]) and np.array_equal(got[key], rowwise("cpso-gamma0")[key]), key
    assert "sweep" not in rowwise("cpso-gamma0")


# ---- 2. it is also the resident batch
@pytest.mark.parametrize("tag", ["de-n65-P17", "de-random-rand2bin", "pso-n64-P16", "pso-shrink-n24"])
def test_it_is_the_resident_factory_batch(sa, tag):
    method, objective, n, P, R, seed, _, opts = _case(tag)
    o = dict(opts, popsize=P, seed=seed, rng="philox", updating="deferred", backend="hip", runs=R)
    ref = sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n), method=method, options=o)
    got = rowwise(tag)
    for key in ("xs", "funs", "nits", "statuses"):
        assert np.array_equal(got[key], ref[key]), key
    assert (got.run, got.nfev, got.fun) == (ref.run, ref.nfev, ref.fun) and np.array_equal(got.x, ref.x)


# ---- 3. runs stop on their own, and stay frozen while the others go on
@pytest.mark.parametrize("tag", STOPPERS)
def test_runs_stop_on_their_own(sa, tag):
    _, _, _, P, R, _, _, _ = _case(tag)
    got = rowwise(tag)
    print("nits", got.nits.tolist(), "statuses", got.statuses.tolist())
    check_runs(got, [single(tag, r) for r in range(R)], P)
    assert len(set(got.nits.tolist())) >= 2      # the runs did not stop together ...
    assert (got.statuses >= 0).any()             # ... and not because the generations ran out
    assert (got.nits < 400).any()
    short = rowwise(tag, maxiter=5)
    assert (short.statuses == -1).all() and (short.nits == 5).all()
    for r in range(0, R, 16):
        one = single(tag, r, maxiter=5)
        assert np.array_equal(short.xs[r], one.x) and short.funs[r] == one.fun and (one.nit, one.status) == (5, -1)


# ---- 4. beyond the LDS
@pytest.mark.parametrize("tag", ["de-beyond-lds", "pso-beyond-lds"])
def test_a_population_the_resident_path_refuses(sa, tag):
    method, objective, n, P, R, seed, _, opts = _case(tag)
    with pytest.raises(ValueError, match="runs.*LDS"):
        sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n), method=method,
                             options=dict(opts, popsize=P, seed=seed, rng="philox", updating="deferred", runs=R))
    check_runs(rowwise(tag), [single(tag, r) for r in range(R)], P)


# ---- 5. non-finite values
@pytest.mark.parametrize("tag", ["de-nonfinite", "pso-nonfinite"])
def test_nan_inf_and_ties(sa, tag):
    import torch

    _, objective, n, P, R, seed, _, _ = _case(tag)
    got = rowwise(tag)
    check_runs(got, [single(tag, r) for r in range(R)], P)
    # the rules do fire on the initial populations (so the start kernel's argmin has met them)
    from stochopy_amd import _device, _rng

    ctx = _device.Context()
    seen = []
    for s in _seeds(seed, R):
        with torch.cuda.stream(ctx.stream):
            lo, hi = ctx.upload(np.full(n, -5.12)), ctx.upload(np.full(n, 5.12))
            X = _rng.philox_latin_hypercube(ctx, ctx.empty((P, n)), 0, P, lo, hi, s)
            seen.append(_fun(objective)(X).cpu().numpy())
    seen = np.concatenate(seen)
    finite = seen[np.isfinite(seen)]
    assert np.isnan(seen).any() and np.isposinf(seen).any() and len(np.unique(finite)) < len(finite)


# ---- 6. what f sees
@pytest.mark.parametrize("method", ["de", "pso"])
def test_what_the_objective_sees(sa, method):
    import torch

    from stochopy_amd.optimize._population import _PopulationRun

    R, P, n = 5, 12, 7
    inner, calls, marker = device_fun("sphere"), [], object()

    def fun(X, a, b):
        calls.append((tuple(X.shape), X.dtype, X.is_contiguous(), X.is_cuda, a is marker, b))
        return inner(X)

    res = sa.optimize.minimize(sa.factory.batched(fun, rowwise=True), _bounds(n), args=(marker, 2.5), method=method,
                               options={"runs": R, "popsize": P, "seed": 3, "maxiter": 40, "rng": "philox", "updating": "deferred"})
    assert all(c == ((R * P, n), torch.float64, True, True, True, 2.5) for c in calls)
    assert res.nits.max() <= len(calls) <= res.nits.max() + _PopulationRun.CHECK_EVERY
    assert _PopulationRun.CHECK_EVERY == 32


# ---- 7. a user-written torch objective with args
@pytest.mark.parametrize("method,constraints", [("de", None), ("de", "Random"), ("pso", None), ("pso", "Shrink")])
def test_a_torch_objective_with_args(sa, method, constraints):
    import torch

    R, P, n = 4, 18, 9
    w = torch.linspace(0.5, 2.0, n, dtype=torch.float64, device="cuda")
    o = {"popsize": P, "maxiter": 15, "rng": "philox", "updating": "deferred", "constraints": constraints}
    got = sa.optimize.minimize(sa.factory.batched(weighted_quadratic, rowwise=True), _bounds(n), args=(w, 0.75), method=method,
                               options=dict(o, runs=R, seed=50))
    singles = [sa.optimize.minimize(sa.factory.batched(weighted_quadratic), _bounds(n), args=(w, 0.75), method=method,
                                    options=dict(o, seed=50 + r)) for r in range(R)]
    check_runs(got, singles, P)


# ---- 8. a sweep
DE_SWEEP = {"mutation": [0.3, 0.5, 0.8, 1.2, 0.5, 0.9, 0.4], "recombination": [0.9, 0.5, 0.7, 1.0, 0.2, 0.9, 0.6],
            "strategy": ["best1bin", "rand1bin", "rand2bin", "best2bin", "rand1bin", "best1bin", "rand2bin"]}
PSO_SWEEP = {"inertia": [0.4, 0.6, 0.7298, 0.9, 0.5, 0.7, 0.8], "cognitivity": [0.5, 1.49618, 2.0, 3.0, 1.0, 1.5, 2.5],
             "sociability": [3.0, 2.0, 1.49618, 0.5, 1.0, 2.5, 1.5]}


def _swept(sa, method, swept, R, **options):
    n, P = 10, 16
    o = dict(options, popsize=P, maxiter=12, rng="philox", updating="deferred")
    tiled = {k: [v[r % len(v)] for r in range(R)] for k, v in swept.items()}
    return sa.optimize.minimize(sa.factory.batched(device_fun("rosenbrock"), rowwise=True), _bounds(n), method=method,
                                options=dict(o, runs=R, seed=70, **tiled)), o, n, P


@pytest.mark.parametrize("method,swept", [("de", DE_SWEEP), ("pso", PSO_SWEEP)])
def test_a_sweep_is_the_single_runs(sa, method, swept):
    got, o, n, P = _swept(sa, method, swept, 7)
    assert sorted(got.sweep) == sorted(swept)
    for name, values in swept.items():
        assert list(got.sweep[name]) == list(values), name
    singles = [sa.optimize.minimize(sa.factory.batched(device_fun("rosenbrock")), _bounds(n), method=method,
                                    options=dict(o, seed=70 + r, **{k: v[r] for k, v in swept.items()})) for r in range(7)]
    check_runs(got, singles, P)
    many, _, _, _ = _swept(sa, method, swept, 300)  # the geometry does not matter
    for key in ("xs", "funs", "nits", "statuses"):
        assert np.array_equal(got[key], many[key][:7]), key


# ---- 9. misuse
def test_misuse_raises_at_the_first_call_and_leaves_the_process_usable(sa):
    import torch

    inner = device_fun("sphere")
    o = {"runs": 3, "popsize": 8, "seed": 1, "maxiter": 5, "rng": "philox", "updating": "deferred"}
    bad = {ValueError: lambda X: inner(X).reshape(-1, 1),
           TypeError: lambda X: inner(X).cpu()}
    for method in ("de", "pso"):
        for error, fun in bad.items():
            calls = []

            def counted(X, fun=fun, calls=calls):
                calls.append(1)
                return fun(X)

            with pytest.raises(error, match="batched objective"):
                sa.optimize.minimize(sa.factory.batched(counted, rowwise=True), _bounds(4), method=method, options=o)
            assert len(calls) == 1
        with pytest.raises(TypeError, match="batched objective"):
            sa.optimize.minimize(sa.factory.batched(lambda X: inner(X).cpu().numpy(), rowwise=True), _bounds(4),
                                 method=method, options=o)
        torch.cuda.synchronize()
        good = sa.optimize.minimize(sa.factory.batched(inner, rowwise=True), _bounds(4), method=method, options=o)
        assert good.xs.shape == (3, 4) and (good.nits == 5).all()
