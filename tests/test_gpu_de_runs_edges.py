"""The batched-runs DE kernel (csrc/sx_de_runs.hip) on WHOLE populations and at its edges, through its C ABI with a real
xfinal buffer (tests/_de_runs_abi.py).  Three references:

(a) the numpy oracle's Philox DE, bit for bit, for the `+ - *` objectives (sphere, rosenbrock: EXACT in test_gpu_de.py):
    the final population after selection (return_all at verbosity 1: xall[-1]), x, fun, nit, status;
(b) the single-run path for all seven objectives: one minimize(rng="philox", updating="deferred") per run, which leaves its
    final population in x0 (test_gpu_edges.py test_x0_population_and_inplace_semantics), bit for bit;
(c) identities of the five outputs among themselves.

Shapes are the smallest at which the kernel takes another path: row lengths around the lanes-per-row and LDS-stride
boundaries and the compile-time summation plans, populations beyond one 64-lane chunk of the best-row search and up to the
160 KiB of LDS, per-dimension bounds, crossover 0 and 1, tied and non-finite fitness, and the status ladder on rows longer
than a wavefront."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _de_runs_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ["ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang"]
EXACT = ("sphere", "rosenbrock")
STRATEGIES = ["rand1bin", "rand2bin", "best1bin", "best2bin"]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(scope="module")
def lib(sa):
    from stochopy_amd import _lib

    return _lib.lib()


def box(n, lo=-5.12, hi=5.12):
    return np.full(n, lo), np.full(n, hi)


def launch(objective, lower, upper, P, seeds, x0=None, want_final=True, **opts):
    """opts in optimize.minimize's spelling."""
    return abi.launch_runs(objective, lower, upper, P, seeds, x0=x0, strategy=opts.get("strategy", "best1bin"),
                           constraints=opts.get("constraints"), maxiter=opts["maxiter"], F=opts.get("mutation", 0.5),
                           CR=opts.get("recombination", 0.9), xtol=opts.get("xtol", 1e-8), ftol=opts.get("ftol", 1e-8),
                           want_final=want_final)


def x0_of(x0, r):
    return None if x0 is None else (x0 if x0.ndim == 2 else x0[r])


def oracle_run(objective, lower, upper, P, seed, x0=None, **opts):
    """The oracle's run and its final population.  return_all allocates `maxiter` slots and the reference always runs two
    generations, so a run of maxiter < 2 hands its population over through the callback instead (the same array)."""
    o = dict(opts, popsize=P, seed=seed, updating="deferred")
    seen, cb = [], None
    if opts["maxiter"] >= 2:
        o.update(return_all=True, verbosity=1.0)
    else:
        cb = lambda X, res: seen.append(np.array(X))  # noqa: E731
    with np.errstate(all="ignore"):
        ref = oracle.minimize(objective, np.stack([lower, upper], axis=1), x0=None if x0 is None else x0.copy(), method="de",
                              options=o, rng="philox", callback=cb)
    return ref, (ref.xall[-1] if cb is None else seen[-1])


def same(a, b, nan=False):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=nan)


def check_oracle(out, objective, lower, upper, P, seeds, x0, opts, nan=False, runs=None):
    """Reference (a)."""
    assert objective in EXACT
    xs, funs, nits, statuses, xfinal = out
    refs = {}
    for r in (range(len(seeds)) if runs is None else runs):
        ref, final = oracle_run(objective, lower, upper, P, seeds[r], x0_of(x0, r), **opts)
        bad = np.flatnonzero(~np.all((xfinal[r] == final) | (np.isnan(final) & np.isnan(xfinal[r]) & nan), axis=1))
        assert same(xfinal[r], final, nan), f"run {r}: rows {bad[:8]} of {P} of the final population differ from the oracle's"
        assert same(xs[r], ref.x, nan), f"run {r}: x"
        assert same(funs[r], ref.fun, nan), f"run {r}: fun {funs[r]!r} != {ref.fun!r}"
        assert (nits[r], statuses[r]) == (ref.nit, ref.status), f"run {r}: nit / status"
        refs[r] = (ref, final)
    return refs


def check_single(sa, out, objective, lower, upper, P, seeds, x0, opts, nan=False, runs=None):
    """Reference (b): the run's own minimize() call, which works in place on its x0."""
    xs, funs, nits, statuses, xfinal = out
    bounds = np.stack([lower, upper], axis=1).tolist()
    for r in (range(len(seeds)) if runs is None else runs):
        pop = x0_of(x0, r).copy()
        one = sa.optimize.minimize(getattr(sa.factory, objective), bounds, x0=pop, method="de",
                                   options=dict(opts, popsize=P, seed=seeds[r], rng="philox", updating="deferred", backend="hip"))
        bad = np.flatnonzero(~np.all((xfinal[r] == pop) | (np.isnan(pop) & np.isnan(xfinal[r]) & nan), axis=1))
        assert same(xfinal[r], pop, nan), f"run {r}: rows {bad[:8]} of {P} of the final population differ from the single run's"
        assert same(xs[r], one.x, nan), f"run {r}: x"
        assert same(funs[r], one.fun, nan), f"run {r}: fun {funs[r]!r} != {one.fun!r}"
        assert (nits[r], statuses[r]) == (one.nit, one.status), f"run {r}: nit / status"


def check_identities(sa, out, objective, nan=False):
    """Reference (c): x is the first-minimum row of the final population, fun its objective value."""
    xs, funs, nits, statuses, xfinal = out
    device = getattr(sa.factory, objective)
    for r in range(len(xs)):
        with np.errstate(all="ignore"):
            f = oracle.OBJECTIVES[objective](xfinal[r]) if objective in EXACT else device(xfinal[r])
        k = int(np.argmin(f))
        assert same(xs[r], xfinal[r][k], nan), f"run {r}: x is not row {k} of the final population"
        assert same(funs[r], device(xs[r][None])[0], nan), f"run {r}: fun is not the objective of x"
        if objective in EXACT:
            assert same(funs[r], f[k], nan)


def identical(a, b):
    return all((u is None and v is None) or (u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes())
               for u, v in zip(a, b))


# --------------------------------------------------------------------------- #
# row lengths: 16 / 32 / 64 lanes per row (64 | 65, 128 | 129), the LDS row stride's two forms (256 | 257), one element,
# the run-time summation plans (300, 2047) and two of the compile-time ones (1024, 2048: at the largest population that fits)
# --------------------------------------------------------------------------- #
ROWS = {  # n: (strategy with sphere, strategy with rosenbrock)
    1: ("best1bin", "rand1bin"), 2: ("rand1bin", "best2bin"), 64: ("rand2bin", "best1bin"), 65: ("best2bin", "rand2bin"),
    128: ("rand1bin", "best1bin"), 129: ("rand2bin", "rand1bin"), 256: ("best2bin", "rand2bin"), 257: ("best1bin", "best2bin"),
    300: ("rand2bin", "rand1bin"), 1024: ("best2bin", "rand2bin"), 2047: ("rand1bin", "best1bin"), 2048: ("best1bin", "rand1bin"),
}


@pytest.mark.parametrize("objective", EXACT)
@pytest.mark.parametrize("n", sorted(ROWS))
def test_row_lengths_against_the_oracle(sa, lib, n, objective):
    from stochopy_amd import _lib

    strategy = ROWS[n][EXACT.index(objective)]
    P = abi.largest_popsize(lib, n) if n >= 1024 else 6 + n % 3  # (9, 4 and 4 rows)
    assert P - 1 >= _lib.DE_DONORS[strategy]
    lower, upper = box(n)
    opts = {"maxiter": 6, "strategy": strategy}
    seeds = [40 + n, 41 + n]
    out = launch(objective, lower, upper, P, seeds, **opts)
    check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)


# --------------------------------------------------------------------------- #
# all seven objectives against the single run, per-run x0; Griewank and Quartic on the long rows whose kernels spill
# --------------------------------------------------------------------------- #
OBJECTIVE_SHAPES = [(objective, n) for objective in ALL for n in (10, 100, 130, 300)] + [("griewank", 512), ("quartic", 1024)]


@pytest.mark.parametrize("objective,n", OBJECTIVE_SHAPES)
def test_objectives_against_the_single_run(sa, lib, objective, n):
    R = 2
    P = min(abi.largest_popsize(lib, n), {10: 17, 100: 12, 130: 9, 300: 8, 512: 8}.get(n, 1 << 20))
    strategy = STRATEGIES[(ALL.index(objective) + n) % 4]
    lower, upper = box(n)
    opts = {"maxiter": 8, "strategy": strategy}
    seeds = [7 + n, 8 + n]
    x0 = np.random.RandomState(n + len(objective)).uniform(-5.12, 5.12, (R, P, n))
    keep = x0.copy()
    out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
    assert np.array_equal(x0, keep)
    check_single(sa, out, objective, lower, upper, P, seeds, x0, opts)
    check_identities(sa, out, objective)
    if objective in EXACT:
        check_oracle(out, objective, lower, upper, P, seeds, x0, opts)


# --------------------------------------------------------------------------- #
# populations beyond one 64-lane chunk of wavefront 0's best-row search, many passes over the rows, the largest that fit
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,P,strategy,objective", [
    (3, 65, "best1bin", "sphere"), (5, 130, "rand2bin", "rosenbrock"), (3, 200, "best1bin", "rosenbrock"),
    (8, 257, "rand2bin", "sphere"), (3, "max", "best1bin", "rosenbrock"), (3, "max", "rand2bin", "sphere"),
    (257, "max", "best1bin", "sphere")])
def test_large_populations_against_the_oracle(sa, lib, n, P, strategy, objective):
    opts = {"maxiter": 5, "strategy": strategy}
    if P == "max":
        P = abi.largest_popsize(lib, n)
        assert abi.lds_bytes(P, n) <= 160 * 1024 < abi.lds_bytes(P + 1, n)
        opts["maxiter"] = 3
    lower, upper = box(n)
    seeds = [300 + n, 500 + P]
    out = launch(objective, lower, upper, P, seeds, **opts)
    check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)


def test_a_best_row_beyond_the_first_chunk(sa):
    """Shared x0 whose best row is row 100 of 130, far below the others: every trial is built around it (best1bin), and it
    is still the best row at the end."""
    n, P = 5, 130
    x0 = np.random.RandomState(2).uniform(2.0, 5.0, (P, n))
    x0[100] = 0.01
    lower, upper = box(n)
    opts = {"maxiter": 3, "strategy": "best1bin"}
    seeds = [1, 2]
    for objective in EXACT:
        out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
        refs = check_oracle(out, objective, lower, upper, P, seeds, x0, opts)
        check_identities(sa, out, objective)
        for _, final in refs.values():  # (the oracle alone: the case is what it is meant to be)
            assert int(np.argmin(oracle.OBJECTIVES[objective](final))) == 100


# --------------------------------------------------------------------------- #
# per-dimension bounds: the Latin hypercube and the Random repair index lower[e] / upper[e]
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("constraints", [None, "Random"])
@pytest.mark.parametrize("objective,strategy", [("sphere", "rand2bin"), ("rosenbrock", "best1bin")])
def test_per_dimension_bounds(sa, objective, strategy, constraints):
    n, P = 70, 33
    i = np.arange(n)
    lower, upper = -1.0 - 0.1 * i, 0.5 + 0.05 * i
    opts = {"maxiter": 12, "strategy": strategy, "mutation": 1.5}
    if constraints:
        opts["constraints"] = constraints
    seeds = [13, 14, 15]
    # the oracle alone: the candidates of the same case without repair leave the box (so repairs happen with it), the
    # candidates with repair never do
    for repair in (None, "Random"):
        seen = []

        def recording(X):
            seen.append(np.array(X))
            return oracle.OBJECTIVES[objective](X)

        oracle.minimize(recording, np.stack([lower, upper], axis=1), method="de", rng="philox",
                        options=dict(opts, constraints=repair, popsize=P, seed=seeds[0], updating="deferred"))
        outside = sum(int(((U < lower) | (U > upper)).sum()) for U in seen)
        assert (outside > 100) if repair is None else (outside == 0), outside
    out = launch(objective, lower, upper, P, seeds, **opts)
    check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)
    if constraints:
        xfinal = out[4]
        assert ((xfinal >= lower) & (xfinal <= upper)).all()


# --------------------------------------------------------------------------- #
# crossover edges: recombination 0 (only the forced index is taken) and 1
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("CR", [0.0, 1.0])
@pytest.mark.parametrize("objective,n,P,strategy", [("sphere", 130, 9, "rand1bin"), ("rosenbrock", 10, 12, "best2bin")])
def test_crossover_edges(sa, objective, n, P, strategy, CR):
    lower, upper = box(n)
    opts = {"maxiter": 8, "strategy": strategy, "recombination": CR}
    seeds = [61, 62, 63]
    out = launch(objective, lower, upper, P, seeds, **opts)
    refs = check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)
    if CR == 0.0:  # a trial differs from its row in one element: so does a final row from the initial one per accepted trial
        ref0, _ = oracle_run(objective, lower, upper, P, seeds[0], None, **dict(opts, maxiter=2))
        changed = (ref0.xall[1] != ref0.xall[0]).sum(axis=1)
        assert changed.max() <= 1


# --------------------------------------------------------------------------- #
# ties: np.argmin's first minimum, within a chunk of 64 rows and across chunks; the kept bits are that row's
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("maxiter", [1, 3])
@pytest.mark.parametrize("tied", [(3, 64, 129), (63, 70), (70, 129)], ids=lambda t: "-".join(map(str, t)))
def test_tied_minimum_rows(sa, tied, maxiter):
    """The tied minimum is f = 0, which a strict `<` cannot beat: the tie is still there when the run ends (generation 2,
    fun = 0 <= ftol), so which row won it is what `xs` shows.  The tied rows are all zeros and differ in the sign of one zero
    each -- the first one has none --, so their bytes tell them apart while sphere() does not."""
    n, P = 5, 130
    x0 = np.random.RandomState(11).uniform(1.0, 5.0, (P, n))
    for k, row in enumerate(tied):
        x0[row] = 0.0
        if k:
            x0[row, k] = -0.0
    if tied[0] == 3:  # another tie that is not the minimum, across the chunk boundary
        x0[63] = x0[70] = [0.5, 0.25, -0.5, 0.25, 0.0]
    first, others = x0[tied[0]].tobytes(), [x0[row].tobytes() for row in tied[1:]]
    assert first not in others and len(set(others)) == len(others)
    lower, upper = box(n)
    opts = {"maxiter": maxiter, "strategy": "best1bin"}
    seeds = [3, 4]
    out = launch("sphere", lower, upper, P, seeds, x0=x0, **opts)
    refs = check_oracle(out, "sphere", lower, upper, P, seeds, x0, opts)
    for r, (ref, final) in refs.items():
        # the oracle alone: the tie survives to the outputs, and numpy gives it to the first row
        f = oracle.OBJECTIVES["sphere"](final)
        assert (ref.nit, ref.fun) == (2, 0.0) and (f[list(tied)] == 0.0).all() and int(np.argmin(f)) == tied[0]
        assert all(final[row].tobytes() == x0[row].tobytes() for row in tied)
        assert np.asarray(ref.x).tobytes() == first
        # bits, not values: -0.0 == 0.0
        assert out[0][r].tobytes() == first, f"run {r}: x is not row {tied[0]}'s bits"
        assert out[0][r].tobytes() not in others
        assert out[4][r].tobytes() == final.tobytes(), f"run {r}: the final population's bits"
        assert out[1][r] == 0.0 and out[2][r] == 2
    check_identities(sa, out, "sphere")


# --------------------------------------------------------------------------- #
# non-finite x0: NaN first, then <, then the lower index (test_gpu_nonfinite.py's rules on this kernel)
# --------------------------------------------------------------------------- #
def poisoned(form, R, P, n):
    x0 = np.random.RandomState(3).uniform(-2.0, 2.0, (R, P, n))
    if form == "nan":
        x0[:, 5, 2] = np.nan
    elif form == "inf":
        x0[:, 3, 1] = np.inf
    elif form == "huge":  # squares overflow to inf
        x0[:, 7, :] = 1e200
    elif form == "nan-row66":  # the first NaN is in the first chunk of 64 rows, another one in the second
        x0[:, 66, 1] = np.nan
        x0[:, 5, 2] = np.nan
    return x0


@pytest.mark.parametrize("objective", EXACT)
@pytest.mark.parametrize("strategy", ["rand1bin", "best1bin"])
@pytest.mark.parametrize("form,P", [("nan", 20), ("inf", 20), ("huge", 20), ("nan-row66", 70)])
def test_nonfinite_x0(sa, form, P, strategy, objective):
    R, n = 2, 6
    x0 = poisoned(form, R, P, n)
    lower, upper = box(n, -2.0, 2.0)
    opts = {"maxiter": 8, "strategy": strategy}
    seeds = [21, 22]
    out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
    refs = check_oracle(out, objective, lower, upper, P, seeds, x0, opts, nan=True)
    check_single(sa, out, objective, lower, upper, P, seeds, x0, opts, nan=True)
    check_identities(sa, out, objective, nan=True)
    if form.startswith("nan"):  # numpy's rules: the first NaN row is the best row and is never replaced
        for r, (ref, final) in refs.items():
            assert np.isnan(ref.fun) and same(ref.x, x0[r, 5], nan=True) and ref.status == -1
            assert np.isnan(out[1][r]) and same(out[4][r][5], x0[r, 5], nan=True)


# --------------------------------------------------------------------------- #
# the status ladder on whole-wave rows: dx is select_finalize_kernel's 256-thread summation played by one wavefront
# --------------------------------------------------------------------------- #
def test_status_ladder_on_whole_wave_rows(sa):
    """xtol chosen on the CPU with the oracle: the 16 deciding steps ||xbest_prev - xbest|| lie between 2.39e-3 and 5.25e-3;
    4.3e-3 sits in their widest central gap (4.211e-3 | 4.450e-3: 2.1 % and 3.4 % away), 8 runs end with status 0 and 8
    with status 1, after 2 to 9 generations."""
    n, P, R = 130, 16, 16
    xtol = 4.3e-3
    x0 = np.random.RandomState(5).uniform(-1e-3, 1e-3, (R, P, n))
    lower, upper = box(n)
    opts = {"maxiter": 200, "strategy": "best1bin", "ftol": 2e-5, "xtol": xtol}
    seeds = list(range(100, 100 + R))
    # the oracle alone
    status, margin = [], []
    for r in range(R):
        ref, _ = oracle_run("sphere", lower, upper, P, seeds[r], x0[r], **opts)
        before, after = ref.xall[-2], ref.xall[-1]
        dx = np.linalg.norm(before[np.argmin(oracle.OBJECTIVES["sphere"](before))] - after[np.argmin(oracle.OBJECTIVES["sphere"](after))])
        assert ref.status == (0 if dx <= xtol else 1) and ref.fun <= opts["ftol"] and ref.nit < opts["maxiter"]
        status.append(ref.status)
        margin.append(abs(dx - xtol) / xtol)
    print("statuses", status, "smallest margin of dx to xtol %.4f" % min(margin))
    assert status.count(0) >= 4 and status.count(1) >= 4
    assert min(margin) > 0.01
    out = launch("sphere", lower, upper, P, seeds, x0=x0, **opts)
    check_oracle(out, "sphere", lower, upper, P, seeds, x0, opts)
    four = [status.index(0), R - 1 - status[::-1].index(0), status.index(1), R - 1 - status[::-1].index(1)]
    check_single(sa, out, "sphere", lower, upper, P, seeds, x0, opts, runs=four)
    check_identities(sa, out, "sphere")
    # and the bottom rung: the same runs cut short end with -1 at maxiter
    short = launch("sphere", lower, upper, P, seeds, x0=x0, **dict(opts, maxiter=2, ftol=1e-30))
    assert (short[3] == -1).all() and (short[2] == 2).all()
    check_oracle(short, "sphere", lower, upper, P, seeds, x0, dict(opts, maxiter=2, ftol=1e-30), runs=[0, R - 1])


# --------------------------------------------------------------------------- #
# ABI corners
# --------------------------------------------------------------------------- #
def test_one_run_is_the_single_run(sa):
    n, P = 33, 11
    x0 = np.random.RandomState(8).uniform(-5.12, 5.12, (P, n))
    lower, upper = box(n)
    opts = {"maxiter": 9, "strategy": "rand1bin"}
    for objective in ("rosenbrock", "rastrigin"):
        out = launch(objective, lower, upper, P, [77], x0=x0, **opts)
        assert out[0].shape == (1, n) and out[4].shape == (1, P, n)
        check_single(sa, out, objective, lower, upper, P, [77], x0, opts)
        check_identities(sa, out, objective)
    check_oracle(launch("rosenbrock", lower, upper, P, [77], x0=x0, **opts), "rosenbrock", lower, upper, P, [77], x0, opts)


def test_shared_x0_same_start_different_runs(sa):
    n, P, R = 20, 12, 3
    x0 = np.random.RandomState(9).uniform(-5.12, 5.12, (P, n))
    keep = x0.copy()
    lower, upper = box(n)
    opts = {"maxiter": 6, "strategy": "best2bin"}
    seeds = [5, 6, 7]
    shared = launch("rosenbrock", lower, upper, P, seeds, x0=x0, **opts)            # x0_stride = 0
    assert np.array_equal(x0, keep)
    check_oracle(shared, "rosenbrock", lower, upper, P, seeds, x0, opts)
    assert not np.array_equal(shared[4][0], shared[4][1]) and not np.array_equal(shared[4][1], shared[4][2])
    assert len(set(shared[1].tolist())) == R
    tiled = launch("rosenbrock", lower, upper, P, seeds, x0=np.tile(x0, (R, 1, 1)), **opts)  # x0_stride = P n
    assert identical(shared, tiled)


@pytest.mark.parametrize("n,P,R", [(3, 4, 300), (128, 64, 2)])
def test_same_launch_twice_same_bytes(sa, n, P, R):
    lower, upper = box(n)
    opts = {"maxiter": 10, "strategy": "best1bin"}
    seeds = list(range(1000, 1000 + R))
    first = launch("rosenbrock", lower, upper, P, seeds, **opts)
    second = launch("rosenbrock", lower, upper, P, seeds, **opts)
    assert identical(first, second)
    check_oracle(first, "rosenbrock", lower, upper, P, seeds, None, opts, runs=sorted({0, R // 2, R - 1}))
    without = launch("rosenbrock", lower, upper, P, seeds, want_final=False, **opts)
    assert without[4] is None and identical(first[:4], without[:4])
