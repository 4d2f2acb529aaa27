"""DE with options["runs"] = R on the GPU (csrc/sx_de_runs.hip: one resident workgroup per run): run r of a batched call is
the single run of seed s + r through the chained generation kernels -- same draws, same arithmetic, same orders of summation,
so the same bits --, runs stop on their own, the launch geometry does not matter, and two of the shapes are also held against
the numpy oracle's Philox DE."""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SPAN = 10.24


def _bounds(n):
    return [[-5.12, 5.12]] * n


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def _x0(kind, R, P, n):
    if kind is None:
        return None
    rs = np.random.RandomState(5)
    return rs.uniform(-5.12, 5.12, (P, n) if kind == "shared" else (R, P, n))


# tag: (objective, n, popsize, runs, seed, x0 kind, options)
CASES = {
    # fewer elements than lanes, best1bin's smallest population (also held against the oracle)
    "n3-P4": ("rosenbrock", 3, 4, 2, 7, None, {"maxiter": 12, "strategy": "best1bin"}),
    # more runs than the device has CUs
    "n3-P4-R300": ("sphere", 3, 4, 300, 1000, None, {"maxiter": 12, "strategy": "best1bin"}),
    # the last row length of 16 lanes per row; one pass of 16 rows exactly
    "n64-P16": ("rosenbrock", 64, 16, 3, 21, None, {"maxiter": 20, "strategy": "rand1bin"}),
    # the first of 32 lanes per row; one row more than two passes of 8 (also held against the oracle)
    "n65-P17": ("rosenbrock", 65, 17, 3, 3, None, {"maxiter": 15, "strategy": "best1bin"}),
    "n64-P4-cos": ("rastrigin", 64, 4, 3, 11, None, {"maxiter": 25, "strategy": "best1bin"}),
    "n128-P16": ("sphere", 128, 16, 2, 5, None, {"maxiter": 12, "strategy": "best2bin"}),
    # whole-wave rows with a ragged last row step, rand2bin's smallest population
    "n130-P6": ("rastrigin", 130, 6, 3, 8, None, {"maxiter": 12, "strategy": "rand2bin"}),
    # several four-step batches; the objective's terms are formed inside the reduction
    "n300-P16": ("rosenbrock", 300, 16, 2, 2, None, {"maxiter": 12, "strategy": "rand1bin"}),
    "n300-P16-cos": ("ackley", 300, 16, 2, 4, None, {"maxiter": 12, "strategy": "best1bin"}),
    # a long row of one of the lengths whose summation plan is a compile-time constant
    "n512-P8": ("rosenbrock", 512, 8, 2, 6, None, {"maxiter": 6, "strategy": "best1bin"}),
    # three passes of 16 rows, the last one ragged
    "n32-P40": ("ackley", 32, 40, 3, 9, None, {"maxiter": 30, "strategy": "best1bin"}),
    "n10-P17": ("griewank", 10, 17, 2, 12, None, {"maxiter": 20, "strategy": "rand1bin"}),
    # more than the default limit of dynamic LDS; eight wavefronts
    "n128-P40": ("griewank", 128, 40, 2, 14, None, {"maxiter": 12, "strategy": "best1bin"}),
    "n128-P64": ("rosenbrock", 128, 64, 2, 15, None, {"maxiter": 12, "strategy": "rand1bin"}),
    # Random with a mutation factor that throws candidates out of the box: repairs happen
    "random-rand2bin": ("sphere", 70, 33, 3, 13, None,
                        {"maxiter": 12, "strategy": "rand2bin", "constraints": "Random", "mutation": 1.5}),
    "random-best2bin": ("rastrigin", 24, 40, 2, 16, None,
                        {"maxiter": 15, "strategy": "best2bin", "constraints": "Random", "mutation": 1.5}),
    # maxiter <= 1 still runs one generation; two generations
    "maxiter1": ("rosenbrock", 10, 16, 3, 17, None, {"maxiter": 1}),
    "maxiter2": ("sphere", 65, 6, 2, 18, None, {"maxiter": 2, "strategy": "rand2bin"}),
    # unrelated seeds, one of them beyond 32 bits (both key words)
    "seed-sequence": ("rosenbrock", 32, 32, 3, (977, 3, (1 << 40) + 17), None, {"maxiter": 60}),
    "x0-shared": ("sphere", 8, 16, 3, 19, "shared", {"maxiter": 25}),
    "x0-per-run": ("rosenbrock", 130, 17, 2, 20, "per-run", {"maxiter": 10, "strategy": "rand1bin"}),
}


def _case(tag):
    return STOP if tag == "stop" else CASES[tag]


def _seeds(seed, R):
    return list(seed) if isinstance(seed, tuple) else [seed + r for r in range(R)]


@functools.lru_cache(maxsize=None)
def batched(tag, runs=None, **changes):
    import stochopy_amd as sa

    objective, n, P, R, seed, x0kind, opts = _case(tag)
    R = runs or R
    o = dict(opts, popsize=P, seed=list(seed) if isinstance(seed, tuple) else seed, rng="philox", updating="deferred",
             backend="hip", runs=R, **changes)
    x0 = _x0(x0kind, R, P, n)
    keep = None if x0 is None else x0.copy()
    res = sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n), x0=x0, method="de", options=o)
    assert keep is None or np.array_equal(x0, keep)  # x0 is not modified
    return res


@functools.lru_cache(maxsize=None)
def single(tag, r, **changes):
    """Run r of the case through today's path: one minimize() call of its own."""
    import stochopy_amd as sa

    objective, n, P, R, seed, x0kind, opts = _case(tag)
    s = seed[r] if isinstance(seed, tuple) else seed + r
    o = dict(opts, popsize=P, seed=s, rng="philox", updating="deferred", backend="hip", **changes)
    x0 = _x0(x0kind, R, P, n)
    if x0 is not None:
        x0 = (x0 if x0kind == "shared" else x0[r]).copy()  # (a single run works in place on x0)
    return sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n), x0=x0, method="de", options=o)


def check_runs(got, singles, P):
    R = len(singles)
    assert got.xs.shape == (R, len(singles[0].x)) and got.funs.shape == got.nits.shape == got.statuses.shape == (R,)
    for r, one in enumerate(singles):
        assert np.array_equal(got.xs[r], one.x), f"run {r}: x"
        assert got.funs[r] == one.fun, f"run {r}: fun {got.funs[r]!r} != {one.fun!r}"
        assert got.nits[r] == one.nit and got.statuses[r] == one.status, \
            f"run {r}: nit / status {got.nits[r]}, {got.statuses[r]} != {one.nit}, {one.status}"
    b = int(np.argmin(got.funs))
    assert got.run == b and np.array_equal(got.x, got.xs[b]) and got.fun == got.funs[b]
    assert got.nit == got.nits[b] and got.status == got.statuses[b] and got.success == (got.status >= 0)
    assert got.message == singles[b].message
    assert got.nfev == int(got.nits.sum()) * P


@pytest.mark.parametrize("tag", sorted(CASES))
def test_run_r_is_the_single_run_bit_for_bit(sa, tag):
    _, _, P, R, _, _, _ = CASES[tag]
    check_runs(batched(tag), [single(tag, r) for r in range(R)], P)


# the shape tests/test_gpu_external.py uses to reach status 0 / 1, under 64 seeds
STOP = ("sphere", 4, 32, 64, 13, None, {"maxiter": 400, "ftol": 1e-6, "xtol": 1e-3})


def test_runs_stop_on_their_own(sa):
    _, _, P, R, _, _, _ = STOP
    got = batched("stop")
    print("nits", got.nits.tolist(), "statuses", got.statuses.tolist())
    check_runs(got, [single("stop", r) for r in range(R)], P)
    assert len(set(got.nits.tolist())) >= 2      # the runs did not stop together ...
    assert (got.statuses >= 0).any()             # ... and not because the generations ran out
    assert (got.nits < 400).any()
    short = batched("stop", maxiter=5)
    assert (short.statuses == -1).all() and (short.nits == 5).all()
    for r in range(0, R, 16):
        one = single("stop", r, maxiter=5)
        assert np.array_equal(short.xs[r], one.x) and short.funs[r] == one.fun and (one.nit, one.status) == (5, -1)


def test_launch_geometry_does_not_matter(sa):
    few, many = batched("n3-P4-R300", runs=7), batched("n3-P4-R300")
    assert many.xs.shape[0] == 300
    for key in ("xs", "funs", "nits", "statuses"):
        assert np.array_equal(few[key], many[key][:7]), key
    assert np.array_equal(few.xs[5], many.xs[5]) and few.funs[5] == many.funs[5]


@pytest.mark.parametrize("tag", ["n3-P4", "n65-P17"])
def test_against_the_oracle(sa, tag):
    objective, n, P, R, seed, _, opts = CASES[tag]
    got = batched(tag)
    for r, s in enumerate(_seeds(seed, R)):
        ref = oracle.minimize(objective, _bounds(n), method="de",
                              options=dict(opts, popsize=P, seed=s, updating="deferred"), rng="philox")
        assert (got.nits[r], got.statuses[r]) == (ref.nit, ref.status)
        assert np.allclose(got.xs[r], ref.x, rtol=0, atol=1e-6 * SPAN), f"run {r}"
        assert np.isclose(got.funs[r], ref.fun, rtol=1e-6, atol=0), f"run {r}"
