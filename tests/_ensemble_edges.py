"""The case tables of tests/test_gpu_sample_ensemble_edges.py (and of its host twin tests/test_sample_ensemble_edges_host.py):
plain data, numpy and the numpy restatements (tests/_ensemble_oracle.py, tests/_ensemble_moves_oracle.py) -- importable
without a GPU.

The resident ensemble kernels (csrc/sx_sample_ensemble.hip ensemble_kernel<FUN, LPR>, csrc/sx_sample_ensemble_moves.hip
ensemble_moves_kernel<FUN, LPR>) keep an ensemble of W walkers in one workgroup's LDS and walk the active half h = W / 2 in
passes of 16 row groups; a row group has LPR = 16 / 32 lanes for n <= 64 / <= 128 and element e sits in lane e % LPR.  The
objective of a proposal is taken inside `if (i < h)`: under wave divergence wherever h is no multiple of the rows of a wave.
The tables put cases where the lanes, the passes and the LDS sizes change.

Every run draws with rng="philox" inside [-5.12, 5.12]^n.  "Both kernels": KERNELS, stretch=2.0 without moves (ensemble_kernel)
and moves=FOUR (ensemble_moves_kernel).  Tolerances are the ensemble tests': samples within XTOL = 1e-9 of the range, values
within FTOL = 1e-6 relative, counts exact.  A case's seed is the first from its own on that the restatement admits
(_ensemble_cases.admitted, _ensemble_moves_cases.admitted); it is searched HERE, never skipped at run time.  The references
are cached per case so that the host and the GPU file share one evaluation.
"""
import functools

import numpy as np

import _ensemble_cases
import _ensemble_moves_cases
import _ensemble_moves_oracle
import _ensemble_oracle
from oracle import objectives

ALL = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")
LOWER, UPPER = -5.12, 5.12
SPAN = UPPER - LOWER
XTOL, FTOL = 1.0e-9, 1.0e-6
FOUR = [("stretch", 0.25), ("de", 0.25), ("de", 0.25, 1.0), ("snooker", 0.25)]  # (tests/test_gpu_sample_ensemble_moves.py)
PAIR = [("de", 0.5), ("snooker", 0.5)]  # the two moves that combine walkers by differences
KERNELS = ("stretch", "moves")
LDS_LIMIT = 160 * 1024


def bounds(n):
    return [[LOWER, UPPER]] * n


def lanes_per_row(n):
    return 16 if n <= 64 else 32


def lds_bytes(W, n):
    """sx_sample_ensemble_lds_bytes restated (the GPU file compares it with the entry point): the walkers, their values, and
    one staging row of n + 8 doubles per row group -- at most 16 row groups, 4 or 2 to a wave."""
    assert 1 <= n <= 128 and W % 2 == 0 and W >= 4 and W >= 2 * n
    rpw = 64 // lanes_per_row(n)
    rows = rpw * min(16 // rpw, -(-(W // 2) // rpw))
    return 8 * (W * n + W + rows * (n + 8))


def passes(W, n):
    """(passes per half-sweep, rows of the last one)."""
    rpw = 64 // lanes_per_row(n)
    rows = rpw * min(16 // rpw, -(-(W // 2) // rpw))
    h = W // 2
    return -(-h // rows), h - (-(-h // rows) - 1) * rows


def largest_walkers(n, limit=LDS_LIMIT):
    """The largest even W with lds_bytes(W, n) <= limit."""
    W = max(4, 2 * n)
    assert lds_bytes(W, n) <= limit
    step = 1 << 20
    while step >= 2:
        while lds_bytes(W + step, n) <= limit:
            W += step
        step //= 2
    return W


def kernel_options(kernel):
    return {"stretch": 2.0} if kernel == "stretch" else {"moves": FOUR}


def restatement(opts):
    return _ensemble_moves_oracle if any(k in opts for k in ("moves", "burn", "thin")) else _ensemble_oracle


def restate(fun, n, x0, opts, **kwargs):
    with np.errstate(all="ignore"):
        return restatement(opts).sample(fun, bounds(n), x0=x0, options=dict(opts), **kwargs)


def flat(fun, n):
    """rosenbrock has no term at n = 1: it is 0.0 everywhere, and with n - 1 = 0 every d is exactly 0.0."""
    return fun == "rosenbrock" and n == 1


def admit(fun, n, x0, opts, tries=8):
    """(seed, the restated run) by the existing admission of the restatement that serves ``opts``.

    The flat case cannot pass that function, whatever the seed: it compares the values RELATIVELY, and a 0.0 moved by one unit
    in the last place is 4.9e-324.  Its own seed is admitted by the same nudges with the values compared absolutely (they stay
    below 1e-300), the samples within XTOL of the range and the counts exactly."""
    cases = _ensemble_moves_cases if restatement(opts) is _ensemble_moves_oracle else _ensemble_cases
    if not flat(fun, n):
        return cases.admitted(fun, bounds(n), x0, dict(opts), tries=tries)
    rs = np.random.RandomState(0)

    def nudge(v):
        v = np.asarray(v, dtype=np.float64)
        return np.nextafter(v, v + rs.choice([-1.0, 1.0], size=v.shape))

    extra = {"nudge": nudge} if restatement(opts) is _ensemble_moves_oracle else {}
    for seed in range(opts["seed"], opts["seed"] + tries):
        o = dict(opts, seed=seed)
        a = restate(fun, n, x0, o)
        b = restate(lambda X: nudge(objectives.OBJECTIVES[fun](X)), n, x0, o, **extra)
        assert not a.funall.any() and np.all(np.abs(b.funall) < 1e-300)
        if np.array_equal(a.nacc, b.nacc) and np.array_equal(a.nfeas, b.nfeas) and np.max(np.abs(a.xall - b.xall)) <= XTOL * SPAN:
            return seed, a
    raise AssertionError("no admissible seed")


def agrees(got, want):
    """The ensemble tests' parities between two runs: counts exact, samples within XTOL of the range, values within FTOL."""
    same = np.array_equal(got.accept_ratios, want.accept_ratios) and got.accept_ratio == want.accept_ratio
    return bool(same and np.allclose(got.xall, want.xall, rtol=0, atol=XTOL * SPAN, equal_nan=True)
                and np.allclose(got.funall, want.funall, rtol=FTOL, atol=0, equal_nan=True)
                and np.allclose(got.x, want.x, rtol=0, atol=XTOL * SPAN, equal_nan=True)
                and np.allclose(got.fun, want.fun, rtol=FTOL, atol=0, equal_nan=True))


# ---- A. every objective at every row width, resident kernels --------------------------------------------------------------
# W = 2 n + 4 where the LDS admits it: h = 5, 10 leave idle row groups in the last wave; h = 18, 19, 34, 35, 66, 67 end in a
# ragged pass of 2 or 3 rows; n = 65, 96: 32-lane rows; n = 96 stays at W = 192 (196 would take 161.5 KiB); n = 1: W = 6, so the
# snooker entry is legal.
A_NS = (1, 3, 8, 16, 17, 32, 33, 64, 65, 96)
A_ENSEMBLES, A_MAXITER = 3, 30
A_CASES = tuple((name, n, kernel) for kernel in KERNELS for n in A_NS for name in ALL)
A_BLIND = (16, 32)  # the first elements of a lane's second and third trip (16-lane rows), next to element n - 1


def case_id(case):
    return "-".join(str(v) for v in case)


def a_walkers(n):
    return 2 * n + 4 if lds_bytes(2 * n + 4, n) <= LDS_LIMIT else 2 * n


def a_options(case):
    name, n, kernel = case
    o = dict({"maxiter": A_MAXITER, "walkers": a_walkers(n), "chains": A_ENSEMBLES, "seed": 700 + n}, **kernel_options(kernel))
    if flat(name, n):
        # every d is 0.0 and accepts: left alone the walkers are a free random walk (the snooker move takes them to 1e13 within
        # the 30 samples, where 1e-9 of the range is below one unit in the last place and no seed is admitted).  "Reject" keeps
        # them in the box, and the proposals that leave it are the case's rejections
        o["constraints"] = "Reject"
    return o


@functools.lru_cache(maxsize=None)
def a_reference(case):
    name, n, _ = case
    return admit(name, n, None, a_options(case))


def blind_elements(n):
    return tuple(sorted({e for e in (n - 1,) + A_BLIND if e < n}))


def blinded(name, e):
    """The objective ``name`` of a kernel that lost element e: it reads 0.0 in its place."""
    f = objectives.OBJECTIVES[name]

    def fun(X):
        X = np.array(X, dtype=np.float64, copy=True)
        X[:, e] = 0.0
        return f(X)

    return fun


def a_discriminates(case, e, samples=3):
    """Whether the restated run of the case at its admitted seed with the objective blind to element e leaves the reference by
    more than the tolerances within its first ``samples`` samples (a run of fewer samples is the beginning of the longer one:
    what differs there differs in the 30)."""
    name, n, _ = case
    seed, want = a_reference(case)
    got = restate(blinded(name, e), n, None, dict(a_options(case), seed=seed, maxiter=samples))
    return not (np.allclose(got.xall, want.xall[:, :samples], rtol=0, atol=XTOL * SPAN)
                and np.allclose(got.funall, want.funall[:, :samples], rtol=FTOL, atol=0))


# ---- B. W far above 2 n, and the 64 KiB line -------------------------------------------------------------------------------
B_ENSEMBLES, B_MAXITER, B_SEED = 2, 12, 5
B_LARGEST = {n: largest_walkers(n) for n in (1, 8, 33)}  # 10168 (318 passes per half-sweep), 2246, 582
B_LINE = (largest_walkers(16, 64 * 1024), largest_walkers(16, 64 * 1024) + 2)  # 458 | 460 at n = 16
B_SHAPES = tuple(B_LARGEST.items()) + tuple((16, W) for W in B_LINE)
B_CASES = tuple((name, n, W, kernel) for kernel in KERNELS for n, W in B_SHAPES for name in ("rastrigin", "ackley"))
B_GEOMETRY = (8, B_LARGEST[8])  # where the bit-for-bit checks under other launch geometries run
B_MANY = 9


def b_options(case):
    name, n, W, kernel = case
    return dict({"maxiter": B_MAXITER, "walkers": W, "chains": B_ENSEMBLES, "seed": B_SEED}, **kernel_options(kernel))


@functools.lru_cache(maxsize=None)
def b_reference(case):
    name, n, _, _ = case
    return admit(name, n, None, b_options(case))


# ---- C. 64-lane rows around a caller's objective ---------------------------------------------------------------------------
C_NS = (129, 256, 257, 600, 1030)
C_ENSEMBLES, C_SEED, C_SCALE = 2, 66, 0.7
C_CASES = tuple((n, kernel) for kernel in KERNELS for n in C_NS)


def c_centre(n):
    return np.linspace(-1.0, 1.0, n)


def c_objective(n):
    centre = c_centre(n)
    return lambda X: (C_SCALE * (X - centre) ** 2).sum(axis=1)


def c_options(case):
    n, kernel = case
    return dict({"maxiter": 4 if n > 600 else 8, "walkers": 2 * n, "chains": C_ENSEMBLES, "seed": C_SEED}, **kernel_options(kernel))


@functools.lru_cache(maxsize=None)
def c_reference(case):
    n, _ = case
    return admit(c_objective(n), n, None, c_options(case))


# ---- D. walkers that coincide ----------------------------------------------------------------------------------------------
D_SHAPES = ((5, 12, "rastrigin"), (17, 38, "ackley"), (65, 134, "griewank"))
D_ENSEMBLES, D_MAXITER = 4, 20
D_CASES = tuple((n, W, name, moves) for n, W, name in D_SHAPES for moves in ("pair", "four"))
D_MOVES = {"pair": PAIR, "four": FOUR}


def d_points(n):
    """p (D_ENSEMBLES, n): no element 0, no two elements equal, another point per ensemble."""
    p = np.random.RandomState(40 + n).uniform(0.25, 4.0, (D_ENSEMBLES, n))
    p *= np.where(np.random.RandomState(41 + n).uniform(size=p.shape) < 0.5, -1.0, 1.0)
    return p


def d_x0_whole(n, W):
    """Every walker of ensemble g on p_g."""
    return np.ascontiguousarray(np.broadcast_to(d_points(n)[:, None, :], (D_ENSEMBLES, W, n)))


def d_x0_half(n, W):
    """Walkers [h, W) of ensemble g on p_g, walkers [0, h) drawn uniformly in the box."""
    x0 = d_x0_whole(n, W)
    x0[:, :W // 2] = np.random.RandomState(42 + n).uniform(LOWER, UPPER, (D_ENSEMBLES, W // 2, n))
    return x0


def d_options(n, W, moves, maxiter=D_MAXITER):
    return {"maxiter": maxiter, "walkers": W, "chains": D_ENSEMBLES, "seed": 300 + n, "moves": D_MOVES[moves]}


@functools.lru_cache(maxsize=None)
def d_whole_reference(case, tries=8):
    """(seed, the restated run).  _ensemble_moves_cases.admitted cannot serve here: it moves the snooker move's dd and pr by one
    unit in the last place, and a dd of exactly 0.0 moved to 4.9e-324 is > 0, which takes the other branch of the guard under
    test.  On coinciding walkers dd and pr are sums of exact zeros -- 0.0 in any order of summation, no rounding to model -- so
    this admission moves the objective values alone, and asks for the same as that function: every count kept, samples within
    XTOL of the range, values within FTOL."""
    n, W, name, moves = case
    f = objectives.OBJECTIVES[name]
    rs = np.random.RandomState(0)

    def moved(X):
        v = np.asarray(f(X), dtype=np.float64)
        return np.nextafter(v, v + rs.choice([-1.0, 1.0], size=v.shape))

    x0 = d_x0_whole(n, W)
    opts = d_options(n, W, moves)
    for seed in range(opts["seed"], opts["seed"] + tries):
        o = dict(opts, seed=seed)
        a, b = restate(name, n, x0, o), restate(moved, n, x0, o)
        if np.array_equal(a.nacc, b.nacc) and np.max(np.abs(a.xall - b.xall)) <= XTOL * SPAN and \
                np.allclose(a.funall, b.funall, rtol=FTOL, atol=0):
            return seed, a
    raise AssertionError("no admissible seed")


@functools.lru_cache(maxsize=None)
def d_half_reference(shape):
    n, W, name = shape
    return admit(name, n, d_x0_half(n, W), d_options(n, W, "pair"))


@functools.lru_cache(maxsize=None)
def d_half_first_sample(shape):
    """The restated run of d_half_reference cut after sample 1: its counts are the decisions of that sample alone."""
    n, W, name = shape
    seed, _ = d_half_reference(shape)
    return restate(name, n, d_x0_half(n, W), dict(d_options(n, W, "pair", maxiter=2), seed=seed))


# ---- E. constraints="Reject" through one planted element -------------------------------------------------------------------
E_PAIRS = ((17, 15), (17, 16), (33, 32), (64, 63), (65, 31), (65, 32), (65, 64), (96, 95))
E_ENSEMBLES, E_MAXITER = 4, 10
E_CASES = tuple((n, e, kernel) for kernel in KERNELS for n, e in E_PAIRS)
E_MARGIN = 1.0e-12  # of the range: no proposal's planted element comes this close to a bound


def e_total(n):
    return E_ENSEMBLES * 2 * n * (E_MAXITER - 1)


def e_x0(n, e):
    """(W, n) shared by the ensembles: zeros but element e, which holds values spread over [0.5, 1 - 1e-9] x UPPER with
    alternating sign, in an order that mixes them over both halves.  Every move combines walkers along lines through them, so
    all other elements stay 0.0: a proposal leaves the box through element e or not at all."""
    W = 2 * n
    x0 = np.zeros((W, n))
    values = UPPER * np.linspace(0.5, 1.0 - 1.0e-9, W) * np.where(np.arange(W) % 2 == 0, 1.0, -1.0)
    x0[:, e] = values[np.random.RandomState(n + e).permutation(W)]
    return x0


def e_options(case):
    n, e, kernel = case
    return dict({"maxiter": E_MAXITER, "walkers": 2 * n, "chains": E_ENSEMBLES, "seed": 41 + n + e, "constraints": "Reject"},
                **kernel_options(kernel))


@functools.lru_cache(maxsize=None)
def e_reference(case):
    """(seed, the restated run, its proposals (2 (E_MAXITER - 1), E_ENSEMBLES n, n): every point the objective is asked for
    after the initial ones, one block per half-sweep)."""
    n, e, _ = case
    seed, want = admit("sphere", n, e_x0(n, e), e_options(case))
    seen = []
    sphere = objectives.OBJECTIVES["sphere"]

    def recording(X):
        seen.append(np.array(X, copy=True))
        return sphere(X)

    again = restate(recording, n, e_x0(n, e), dict(e_options(case), seed=seed))
    assert np.array_equal(again.xall, want.xall) and np.array_equal(again.nfeas, want.nfeas)
    assert len(seen) == 1 + 2 * (E_MAXITER - 1)
    return seed, want, np.stack(seen[1:])


# ---- F. burn and thin where the passes and the 32-lane rows are -------------------------------------------------------------
F_SHAPES = ((17, 38, "ackley"), (65, 134, "griewank"))
F_ENSEMBLES, F_MAXITER = 3, 30
F_CUTS = ((7, 3), (29, 1), (0, 2))


def f_options(shape):
    n, W, name = shape
    return {"maxiter": F_MAXITER, "walkers": W, "chains": F_ENSEMBLES, "seed": 31 + n, "moves": FOUR}


@functools.lru_cache(maxsize=None)
def f_reference(shape):
    n, _, name = shape
    return admit(name, n, None, f_options(shape))
