"""PSO / CPSO with options["runs"] = R on the GPU (csrc/sx_pso_runs.hip: one resident workgroup per run): run r of a batched
call is the single run of seed s + r through the generation kernels (whichever of their forms serves the shape) -- same draws,
same arithmetic, same orders of summation, so the same bits --, CPSO restarts included; runs stop on their own, the launch
geometry does not matter, and four of the cases are also held against the numpy oracle's Philox PSO / CPSO."""
import functools

import numpy as np
import pytest

import oracle
import oracle.engine

pytestmark = pytest.mark.gpu

SHRINK = {"constraints": "Shrink", "inertia": 1.0, "cognitivity": 3.0, "sociability": 3.0}  # particles do leave the box


def _bounds(n, half=5.12):
    return [[-half, half]] * n


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def _x0(kind, R, P, n, half):
    if kind is None:
        return None
    rs = np.random.RandomState(5)
    return rs.uniform(-half, half, (P, n) if kind == "shared" else (R, P, n))


# shape tag: (n, popsize, runs, generations) -- the row lengths at which the single run's generation kernel changes form
SHAPES = {
    "n3-P2": (3, 2, 3, 12),         # the smallest swarm
    "n3-P4-R300": (3, 4, 300, 8),   # more runs than the device has CUs
    "n64-P16": (64, 16, 3, 20),     # FULL, 16 lanes per row; one pass of 16 rows exactly
    "n65-P17": (65, 17, 3, 15),     # the first row length of 32 lanes; a ragged third pass
    "n128-P16": (128, 16, 2, 12),   # FULL, 32 lanes
    "n130-P6": (130, 6, 3, 12),     # the one-batch whole-wave form, ragged last step
    "n200-P9": (200, 9, 2, 10),     # the same, three passes of four rows
    "n256-P8": (256, 8, 2, 12),     # FULL, the whole wave
    "n300-P16": (300, 16, 2, 10),   # several four-step batches; terms formed inside the reduction
    "n512-P8": (512, 8, 2, 6),      # a long row whose summation plan is a compile-time constant
    "n32-P40": (32, 40, 3, 30),     # three passes of 16 rows, the last one ragged
    "n128-P40": (128, 40, 2, 12),   # more than the default limit of dynamic LDS; eight wavefronts
    "n128-P64": (128, 64, 2, 10),   # X, V and pbest beyond 160 KiB: the velocities in the workspace
}
OBJECTIVES = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")

# tag: (method, objective, n, popsize, runs, seed, x0 kind, half-width, options)
CASES = {}
for _k, (_tag, (_n, _P, _R, _g)) in enumerate(sorted(SHAPES.items())):
    # all seven objectives go over the shapes, and every objective meets both constraints
    CASES[_tag] = ("pso", OBJECTIVES[_k % 7], _n, _P, _R, 40 + 3 * _k, None, 5.12, {"maxiter": _g})
    CASES[_tag + "-shrink"] = ("pso", OBJECTIVES[(_k + 3) % 7], _n, _P, _R, 140 + 3 * _k, None, 5.12, dict(SHRINK, maxiter=_g))
CASES.update({
    # held against the oracle as well: one objective of +, -, * only, one with cosines
    "oracle-n3-P4": ("pso", "rosenbrock", 3, 4, 2, 7, None, 5.12, {"maxiter": 12}),
    "oracle-n65-P17": ("pso", "rastrigin", 65, 17, 3, 3, None, 5.12, {"maxiter": 15}),
    # maxiter <= 1 still runs one generation; two generations
    "maxiter1": ("pso", "rosenbrock", 10, 16, 3, 17, None, 5.12, {"maxiter": 1}),
    "maxiter2": ("cpso", "sphere", 65, 6, 2, 18, None, 5.12, {"maxiter": 2}),
    # unrelated seeds, one of them beyond 32 bits (both key words)
    "seed-sequence": ("pso", "rosenbrock", 32, 32, 3, (977, 3, (1 << 40) + 17), None, 5.12, {"maxiter": 30}),
    "x0-shared": ("pso", "sphere", 8, 16, 3, 19, "shared", 5.12, {"maxiter": 25}),
    "x0-per-run": ("cpso", "rosenbrock", 130, 17, 2, 20, "per-run", 5.12, dict(SHRINK, maxiter=10)),
})

# CPSO with restarts that happen (each case: 5 ... 28 restarts per run in the oracle, nw from P - 2 down to 1).
# (sphere n = 130, P = 70: X, V and pbest are 218 400 bytes -- the velocities live in the workspace)
#            objective     n   P  half  maxiter gamma  constraints
RESTARTS = [("sphere", 3, 8, 0.5, 30, 1.0, None),
            ("rastrigin", 10, 17, 0.5, 30, 1.0, None),
            ("rosenbrock", 64, 16, 0.25, 30, 1.0, "Shrink"),
            ("ackley", 65, 40, 0.5, 30, 1.2, None),
            ("sphere", 130, 70, 0.5, 24, 0.8, None),
            ("rastrigin", 128, 16, 0.25, 30, 1.0, "Shrink"),
            ("rosenbrock", 300, 9, 0.25, 20, 1.0, None)]
RESTART_TAGS = []
for _k, (_obj, _n, _P, _half, _g, _gamma, _con) in enumerate(RESTARTS):
    _tag = f"restart-{_obj}-n{_n}-P{_P}"
    RESTART_TAGS.append(_tag)
    _o = {"competitivity": _gamma, "constraints": _con}
    CASES[_tag] = ("cpso", _obj, _n, _P, 2 + _k % 2, 30 + _k, None, _half, dict(_o, maxiter=_g))  # the graph form (>= 16)
    CASES[_tag + "-eager"] = ("cpso", _obj, _n, _P, 2, 30 + _k, None, _half, dict(_o, maxiter=12))

# the shape tests/test_gpu_external.py uses to reach status 0 / 1, under 32 seeds
STOP_OPTS = {"maxiter": 400, "ftol": 1e-6, "xtol": 1e-3}
CASES["stop-pso"] = ("pso", "sphere", 4, 32, 32, 13, None, 5.12, STOP_OPTS)
CASES["stop-cpso"] = ("cpso", "sphere", 4, 32, 32, 13, None, 5.12, STOP_OPTS)


def _seeds(seed, R):
    return list(seed) if isinstance(seed, tuple) else [seed + r for r in range(R)]


@functools.lru_cache(maxsize=None)
def batched(tag, runs=None, **changes):
    import stochopy_amd as sa

    method, objective, n, P, R, seed, x0kind, half, opts = CASES[tag]
    R = runs or R
    o = dict(opts, popsize=P, seed=list(seed) if isinstance(seed, tuple) else seed, rng="philox", updating="deferred",
             backend="hip", runs=R, **changes)
    x0 = _x0(x0kind, R, P, n, half)
    keep = None if x0 is None else x0.copy()
    res = sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n, half), x0=x0, method=method, options=o)
    assert keep is None or np.array_equal(x0, keep)  # x0 is not modified
    return res


@functools.lru_cache(maxsize=None)
def single(tag, r, **changes):
    """Run r of the case through today's path: one minimize() call of its own."""
    import stochopy_amd as sa

    method, objective, n, P, R, seed, x0kind, half, opts = CASES[tag]
    s = seed[r] if isinstance(seed, tuple) else seed + r
    o = dict(opts, popsize=P, seed=s, rng="philox", updating="deferred", backend="hip", **changes)
    x0 = _x0(x0kind, R, P, n, half)
    if x0 is not None:
        x0 = (x0 if x0kind == "shared" else x0[r]).copy()
    return sa.optimize.minimize(getattr(sa.factory, objective), _bounds(n, half), x0=x0, method=method, options=o)


@functools.lru_cache(maxsize=None)
def reference(tag, r, record_beta=False):
    """Run r of the case in the numpy oracle; with record_beta also the smallest Shrink factor the run applied."""
    method, objective, n, P, R, seed, x0kind, half, opts = CASES[tag]
    x0 = _x0(x0kind, R, P, n, half)
    if x0 is not None:
        x0 = (x0 if x0kind == "shared" else x0[r]).copy()
    betas = []
    plain = oracle.engine.shrink_factor

    def recording(X, V, lower, upper):
        beta = plain(X, V, lower, upper)
        betas.append(float(np.min(beta)))
        return beta

    oracle.engine.shrink_factor = recording
    try:
        ref = oracle.minimize(objective, _bounds(n, half), x0=x0, method=method,
                              options=dict(opts, popsize=P, seed=_seeds(seed, R)[r], updating="deferred"), rng="philox")
    finally:
        oracle.engine.shrink_factor = plain
    return (ref, min(betas) if betas else 1.0) if record_beta else ref


def check_runs(got, singles, P, rows=None):
    rows = list(range(len(singles))) if rows is None else rows
    R = got.xs.shape[0]
    assert got.xs.shape == (R, len(singles[0].x)) and got.funs.shape == got.nits.shape == got.statuses.shape == (R,)
    for r, one in zip(rows, singles):
        assert np.array_equal(got.xs[r], one.x), f"run {r}: x"
        assert got.funs[r] == one.fun, f"run {r}: fun {got.funs[r]!r} != {one.fun!r}"
        assert got.nits[r] == one.nit and got.statuses[r] == one.status, \
            f"run {r}: nit / status {got.nits[r]}, {got.statuses[r]} != {one.nit}, {one.status}"
    b = int(np.argmin(got.funs))
    assert got.run == b and np.array_equal(got.x, got.xs[b]) and got.fun == got.funs[b]
    assert got.nit == got.nits[b] and got.status == got.statuses[b] and got.success == (got.status >= 0)
    assert got.nfev == int(got.nits.sum()) * P


PLAIN_TAGS = sorted(t for t in CASES if not t.startswith(("restart-", "stop-")))


@pytest.mark.parametrize("tag", PLAIN_TAGS)
def test_run_r_is_the_single_run_bit_for_bit(sa, tag):
    _, _, _, P, R, _, _, _, opts = CASES[tag]
    rows = list(range(R)) if R <= 32 else sorted(set(range(0, R, 23)) | {R - 1})
    check_runs(batched(tag), [single(tag, r) for r in rows], P, rows)
    if opts.get("constraints") == "Shrink":  # the case does shrink velocities (said by the oracle)
        _, beta = reference(tag, 0, record_beta=True)
        print("smallest Shrink factor in the oracle's run 0:", beta)
        assert beta < 1.0


@pytest.mark.parametrize("tag", RESTART_TAGS)
def test_cpso_runs_restart_like_the_single_run_graph_form(sa, tag):
    _, _, _, P, R, _, _, _, opts = CASES[tag]
    for r in range(R):  # the case must exercise the restart (said by the oracle), or this is a PSO test
        ref = reference(tag, r)
        print(tag, "run", r, "restarts (it, nw):", ref["_restarts"])
        assert len(ref["_restarts"]) >= 5
    assert opts["maxiter"] >= 16  # the single run replays its graph
    check_runs(batched(tag), [single(tag, r) for r in range(R)], P)


@pytest.mark.parametrize("tag", RESTART_TAGS)
def test_cpso_runs_restart_like_the_single_run_eager_form(sa, tag):
    tag += "-eager"
    _, _, _, P, R, _, _, _, _ = CASES[tag]
    print(tag, "restarts (it, nw) of run 0 in the oracle:", reference(tag, 0)["_restarts"])
    check_runs(batched(tag), [single(tag, r) for r in range(R)], P)


@pytest.mark.parametrize("method", ["pso", "cpso"])
def test_runs_stop_on_their_own(sa, method):
    tag = "stop-" + method
    _, _, _, P, R, _, _, _, _ = CASES[tag]
    got = batched(tag)
    print("nits", got.nits.tolist(), "statuses", got.statuses.tolist())
    check_runs(got, [single(tag, r) for r in range(R)], P)
    assert len(set(got.nits.tolist())) >= 2                        # the runs did not stop together ...
    assert (got.statuses == 0).any() and (got.statuses == 1).any()  # ... and in both ways the tolerances offer
    assert (got.nits < 400).all()
    short = batched(tag, maxiter=5)
    assert (short.statuses == -1).all() and (short.nits == 5).all()
    for r in range(0, R, 16):
        one = single(tag, r, maxiter=5)
        assert np.array_equal(short.xs[r], one.x) and short.funs[r] == one.fun and (one.nit, one.status) == (5, -1)


def test_launch_geometry_does_not_matter(sa):
    few, many = batched("n3-P4-R300", runs=7), batched("n3-P4-R300")
    assert many.xs.shape[0] == 300
    for key in ("xs", "funs", "nits", "statuses"):
        assert np.array_equal(few[key], many[key][:7]), key


@pytest.mark.parametrize("tag", ["oracle-n3-P4", "oracle-n65-P17"] + RESTART_TAGS[:2])
def test_against_the_oracle(sa, tag):
    _, objective, n, P, R, seed, _, half, _ = CASES[tag]
    got = batched(tag)
    for r in range(R):
        ref = reference(tag, r)
        assert (got.nits[r], got.statuses[r]) == (ref.nit, ref.status)
        if objective in ("sphere", "rosenbrock"):  # +, -, * only: the same bits
            assert np.array_equal(got.xs[r], ref.x) and got.funs[r] == ref.fun, f"run {r}"
        else:
            assert np.allclose(got.xs[r], ref.x, rtol=0, atol=1e-6 * 2 * half), f"run {r}"
            assert np.isclose(got.funs[r], ref.fun, rtol=1e-6, atol=0), f"run {r}"
