"""The batched-runs PSO / CPSO kernel (csrc/sx_pso_runs.hip) on WHOLE swarms and at its edges, through its C ABI with real
xfinal / pbest_final / pbestfit_final buffers (tests/_pso_runs_abi.py).  Two references:

(a) the single-run path for all seven objectives: the run object optimize.minimize builds (_cpso._PsoRun, autorun=False),
    run to its end, whose X, pbest and pbestfit are then read from the device -- bit for bit;
(b) the numpy oracle's Philox PSO / CPSO, bit for bit, for the `+ - *` objectives (sphere, rosenbrock: EXACT in
    test_gpu_pso.py): the final positions (the oracle hands X to its callback), x, fun, nit, status.

Shapes are the smallest at which the kernel takes another path: row lengths around the lanes-per-row and LDS-stride boundaries
and the compile-time summation plans, swarms beyond one 64-lane chunk of the best-row search and up to the 160 KiB of LDS, a
per-dimension box, tied and non-finite fitness, and the status ladder on rows longer than a wavefront."""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _pso_runs_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu

ALL = ["ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang"]
EXACT = ("sphere", "rosenbrock")
KEYS = {"inertia": 0.7298, "cognitivity": 1.49618, "sociability": 1.49618, "competitivity": None, "constraints": None,
        "xtol": 1e-8, "ftol": 1e-8}
SHRINK = {"constraints": "Shrink", "inertia": 1.0, "cognitivity": 3.0, "sociability": 3.0}


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
    """opts in optimize.minimize's spelling (competitivity None: PSO)."""
    o = dict(KEYS, **opts)
    return abi.launch_runs(objective, lower, upper, P, seeds, x0=x0, maxiter=o["maxiter"], want_final=want_final,
                           **{k: o[k] for k in KEYS})


def x0_of(x0, r):
    return None if x0 is None else (x0 if x0.ndim == 2 else x0[r])


def same(a, b, nan=False):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=nan)


def single_run(objective, lower, upper, P, seed, x0=None, **opts):
    """Reference (a): result, X, pbest, pbestfit of the run optimize.minimize(rng="philox", updating="deferred") performs."""
    import torch

    from stochopy_amd import _lib
    from stochopy_amd.optimize._cpso import _PsoRun

    o = dict(KEYS, **opts)
    run = _PsoRun(_lib.FUN_IDS[objective], lower, upper, None if x0 is None else x0.copy(), int(o["maxiter"]), P,
                  o["inertia"], o["cognitivity"], o["sociability"], o["competitivity"], o["constraints"], o["xtol"], o["ftol"],
                  False, 1.0, None, "philox", seed, 1, autorun=False)
    with torch.cuda.stream(run.ctx.stream):
        try:
            run._run()
            state = [t.cpu().numpy().copy() for t in (run.X, run.pbest, run.pbestfit)]
        finally:
            run.close()
    return (run.result(), *state)


def oracle_run(objective, lower, upper, P, seed, x0=None, **opts):
    """Reference (b): the oracle's run and its final positions (the last array its callback saw: nothing moves after it)."""
    o = {k: v for k, v in dict(opts, popsize=P, seed=seed, updating="deferred").items() if k != "competitivity"}
    method = "cpso" if opts.get("competitivity") else "pso"
    if method == "cpso":
        o["competitivity"] = opts["competitivity"]
    seen = []
    with np.errstate(all="ignore"):
        ref = oracle.minimize(objective, np.stack([lower, upper], axis=1), x0=None if x0 is None else x0.copy(), method=method,
                              options=o, rng="philox", callback=lambda X, res: seen.append(np.array(X)))
    return ref, seen[-1]


def check_single(out, objective, lower, upper, P, seeds, x0, opts, nan=False, runs=None):
    xs, funs, nits, statuses, xfinal, pbest, pbestfit = out
    for r in (range(len(seeds)) if runs is None else runs):
        one, X, pb, pf = single_run(objective, lower, upper, P, seeds[r], x0_of(x0, r), **opts)
        for name, got, want in (("X", xfinal[r], X), ("pbest", pbest[r], pb), ("pbestfit", pbestfit[r][:, None], pf[:, None])):
            bad = np.flatnonzero(~np.all((got == want) | (np.isnan(got) & np.isnan(want) & nan), axis=1))
            assert same(got, want, nan), f"run {r}: rows {bad[:8]} of {P} of the final {name} differ from the single run's"
        assert same(xs[r], one.x, nan), f"run {r}: x"
        assert same(funs[r], one.fun, nan), f"run {r}: fun {funs[r]!r} != {one.fun!r}"
        assert (nits[r], statuses[r]) == (one.nit, one.status), f"run {r}: nit / status"


def check_oracle(out, objective, lower, upper, P, seeds, x0, opts, nan=False, runs=None):
    assert objective in EXACT
    xs, funs, nits, statuses, xfinal, pbest, pbestfit = out
    refs = {}
    for r in (range(len(seeds)) if runs is None else runs):
        ref, final = oracle_run(objective, lower, upper, P, seeds[r], x0_of(x0, r), **opts)
        bad = np.flatnonzero(~np.all((xfinal[r] == final) | (np.isnan(final) & np.isnan(xfinal[r]) & nan), axis=1))
        assert same(xfinal[r], final, nan), f"run {r}: rows {bad[:8]} of {P} of the final positions differ from the oracle's"
        assert same(xs[r], ref.x, nan), f"run {r}: x"
        assert same(funs[r], ref.fun, nan), f"run {r}: fun {funs[r]!r} != {ref.fun!r}"
        assert (nits[r], statuses[r]) == (ref.nit, ref.status), f"run {r}: nit / status"
        refs[r] = (ref, final)
    return refs


def check_identities(sa, out, objective, nan=False):
    """x is the first-minimum row of the final personal bests, fun its value; pbestfit is the objective of pbest."""
    xs, funs, nits, statuses, xfinal, pbest, pbestfit = out
    device = getattr(sa.factory, objective)
    for r in range(len(xs)):
        k = int(np.argmin(pbestfit[r]))
        assert same(funs[r], pbestfit[r][k], nan) and same(xs[r], pbest[r][k], nan), f"run {r}: x / fun are not row {k}'s"
        live = pbestfit[r] != 1.0e30  # (a row re-seeded by the last restart has no value yet)
        assert same(device(pbest[r][live]), pbestfit[r][live], nan), f"run {r}: pbestfit is not the objective of pbest"


def identical(a, b):
    return all((u is None and v is None) or (u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes())
               for u, v in zip(a, b))


# --------------------------------------------------------------------------- #
# row lengths: 16 / 32 / 64 lanes per row (16 | 17 elements in one step, 64 | 65, 128 | 129), the LDS row stride's two forms
# (256 | 257), one element, two of the compile-time summation plans (1024, 2048); two to six rows
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("objective", EXACT)
@pytest.mark.parametrize("n", [1, 16, 17, 64, 65, 128, 129, 256, 257, 1024, 2048])
def test_row_lengths(sa, lib, n, objective):
    P = min(2 + (n + len(objective)) % 5, abi.largest_popsize(lib, n))  # (2048: two rows are all that fit)
    lower, upper = box(n)
    opts = {"maxiter": 6}
    if (n + EXACT.index(objective)) % 2:
        opts.update(SHRINK)
    if n % 3 == 1:
        opts["competitivity"] = 1.0
    seeds = [40 + n, 41 + n]
    out = launch(objective, lower, upper, P, seeds, **opts)
    check_single(out, objective, lower, upper, P, seeds, None, opts)
    check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)


# --------------------------------------------------------------------------- #
# all seven objectives against the single run, per-run x0, whole swarms
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("objective,n", [(objective, n) for objective in ALL for n in (10, 130, 300)])
def test_objectives_against_the_single_run(sa, objective, n):
    R, P = 2, {10: 17, 130: 9, 300: 6}[n]
    lower, upper = box(n)
    opts = {"maxiter": 8, "competitivity": 1.0 if (ALL.index(objective) + n // 10) % 2 else None}
    if ALL.index(objective) % 2:
        opts.update(SHRINK)
    seeds = [7 + n, 8 + n]
    x0 = np.random.RandomState(n + len(objective)).uniform(-5.12, 5.12, (R, P, n))
    keep = x0.copy()
    out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
    assert np.array_equal(x0, keep)
    check_single(out, objective, lower, upper, P, seeds, x0, opts)
    check_identities(sa, out, objective)
    if objective in EXACT:
        check_oracle(out, objective, lower, upper, P, seeds, x0, opts)


# --------------------------------------------------------------------------- #
# swarms beyond one 64-lane chunk of wavefront 0's best-row search, many passes over the rows, the largest that fit (their
# broadcast words are the last bytes of 160 KiB)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,P,objective,gamma", [(3, 65, "sphere", None), (5, 130, "rosenbrock", 1.0),
                                                  (3, "max", "rosenbrock", 1.0), (64, "max", "sphere", None),
                                                  (3, "whole", "sphere", 1.0), (64, "whole", "rosenbrock", None),
                                                  (64, "whole+1", "rosenbrock", 1.0)])
def test_large_swarms(sa, lib, n, P, objective, gamma):
    """max: the largest swarm accepted (velocities in the workspace); whole: the largest whose X, V and pbest are all in the
    LDS; whole+1: the first one whose velocities are not."""
    if P == "max":
        P = abi.largest_popsize(lib, n)
        assert abi.lds_bytes(P, n) <= 160 * 1024 < abi.lds_bytes(P + 1, n) and abi.workspace_bytes(1, P, n) > 0
    elif isinstance(P, str):
        whole = max(p for p in range(2, abi.largest_popsize(lib, n)) if abi.workspace_bytes(1, p, n) == 0)
        assert abi.workspace_bytes(1, whole + 1, n) > 0 and abi.lds_bytes(whole, n) > abi.lds_bytes(whole + 1, n)
        P = whole + (P == "whole+1")
    lower, upper = box(n)
    opts = {"maxiter": 3, "competitivity": gamma}
    seeds = [300 + n, 500 + P]
    out = launch(objective, lower, upper, P, seeds, **opts)
    check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    check_single(out, objective, lower, upper, P, seeds, None, opts, runs=[1])
    check_identities(sa, out, objective)


def test_a_best_row_beyond_the_first_chunk(sa):
    """Shared x0 whose best row is row 100 of 130, far below the others: gbest is that row from the start, and it is still
    the best row at the end."""
    n, P = 5, 130
    x0 = np.random.RandomState(2).uniform(2.0, 5.0, (P, n))
    x0[100] = 0.01
    lower, upper = box(n)
    opts = {"maxiter": 3, "inertia": 0.1, "cognitivity": 0.1, "sociability": 0.1}
    seeds = [1, 2]
    for objective in EXACT:
        out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
        check_oracle(out, objective, lower, upper, P, seeds, x0, opts)
        check_single(out, objective, lower, upper, P, seeds, x0, opts, runs=[0])
        check_identities(sa, out, objective)
        assert (np.argmin(out[6], axis=1) == 100).all()


# --------------------------------------------------------------------------- #
# a per-dimension box: the Latin hypercube, Shrink and the restart's re-seeding index lower[e] / upper[e]
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("objective", EXACT)
def test_per_dimension_box_with_shrink_and_restarts(sa, objective):
    n, P = 70, 17
    i = np.arange(n)
    lower, upper = -0.3 - 0.002 * i, 0.2 + 0.001 * i
    opts = dict(SHRINK, maxiter=30, competitivity=1.0)
    seeds = [13, 14]
    out = launch(objective, lower, upper, P, seeds, **opts)
    refs = check_oracle(out, objective, lower, upper, P, seeds, None, opts)
    for ref, _ in refs.values():  # (the oracle alone: rows are re-seeded in this case)
        assert len(ref["_restarts"]) >= 5
    check_single(out, objective, lower, upper, P, seeds, None, opts)
    check_identities(sa, out, objective)
    # Shrink puts a particle ON the bound it would cross, x + v (b - x) / v: b up to the rounding of three operations on
    # numbers below 1 (a few 1e-16)
    for swarm in (out[4], out[5]):
        assert ((swarm >= lower - 1e-12) & (swarm <= upper + 1e-12)).all()


# --------------------------------------------------------------------------- #
# non-finite x0: NaN first, then <, then the lower index (test_gpu_nonfinite.py's rules on this kernel)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("objective", EXACT)
@pytest.mark.parametrize("gamma", [None, 1.0])
@pytest.mark.parametrize("form,P", [("nan", 20), ("inf", 20), ("nan+inf", 20), ("nan-row66", 70)])
def test_nonfinite_x0(sa, form, P, gamma, objective):
    """A NaN row is np.argmin's best row at once and stays gbest; every particle is then pulled towards NaN and the swarm
    radius is NaN, which is not below delta: a CPSO run with a non-finite particle never restarts (np.max propagates the NaN;
    the oracle says so below), so what is compared is that the batched run does not either -- its final X, pbest and pbestfit
    are the single run's, whose restart kernels ran on those keys (NaN the largest) behind the same NaN radius."""
    R, n = 2, 6
    x0 = np.random.RandomState(3).uniform(-0.5, 0.5, (R, P, n))
    if "nan" in form:
        x0[:, 5, 2] = np.nan
    if "inf" in form:
        x0[:, 3, 1] = np.inf
    if form == "nan-row66":  # the first NaN is in the first chunk of 64 rows, another one in the second
        x0[:, 66, 1] = np.nan
    lower, upper = box(n, -0.5, 0.5)
    opts = {"maxiter": 18, "competitivity": gamma}
    seeds = [21, 22]
    out = launch(objective, lower, upper, P, seeds, x0=x0, **opts)
    refs = check_oracle(out, objective, lower, upper, P, seeds, x0, opts, nan=True)
    check_single(out, objective, lower, upper, P, seeds, x0, opts, nan=True)
    for r, (ref, final) in refs.items():
        assert ref["_restarts"] == []
        if "nan" in form:
            assert np.isnan(ref.fun) and same(ref.x, x0[r, 5], nan=True) and ref.status == -1
            assert np.isnan(out[1][r]) and same(out[5][r][5], x0[r, 5], nan=True)


# --------------------------------------------------------------------------- #
# ties: np.argmin's first minimum, within a chunk of 64 rows and across chunks; the kept bits are that row's
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize("gamma", [None, 1.0])
@pytest.mark.parametrize("tied", [(3, 64, 129), (63, 70), (70, 129)], ids=lambda t: "-".join(map(str, t)))
def test_tied_minimum_rows(sa, tied, gamma):
    """The tied minimum is f = 0, which a strict `<` cannot beat: the tied personal bests are still there when the run ends
    (generation 2, fun = 0 <= ftol), so which row won the tie is what `xs` shows.  The tied rows are all zeros and differ in the
    sign of one zero each -- the first one has none --, so their bytes tell them apart while sphere() does not."""
    n, P = 5, 130
    x0 = np.random.RandomState(11).uniform(1.0, 5.0, (P, n))
    for k, row in enumerate(tied):
        x0[row] = 0.0
        if k:
            x0[row, k] = -0.0
    first, others = x0[tied[0]].tobytes(), [x0[row].tobytes() for row in tied[1:]]
    assert first not in others and len(set(others)) == len(others)
    lower, upper = box(n)
    opts = {"maxiter": 3, "competitivity": gamma}
    seeds = [3, 4]
    out = launch("sphere", lower, upper, P, seeds, x0=x0, **opts)
    refs = check_oracle(out, "sphere", lower, upper, P, seeds, x0, opts)
    check_single(out, "sphere", lower, upper, P, seeds, x0, opts, runs=[0])
    for r, (ref, final) in refs.items():
        assert (ref.nit, ref.fun) == (2, 0.0) and np.asarray(ref.x).tobytes() == first  # the oracle alone
        assert out[0][r].tobytes() == first, f"run {r}: x is not row {tied[0]}'s bits"  # bits, not values: -0.0 == 0.0
        assert out[0][r].tobytes() not in others
        assert all(out[5][r][row].tobytes() == x0[row].tobytes() for row in tied) and (out[6][r][list(tied)] == 0.0).all()
        assert out[1][r] == 0.0 and out[2][r] == 2
    check_identities(sa, out, "sphere")


# --------------------------------------------------------------------------- #
# the status ladder on whole-wave rows: dx is select_finalize_kernel's 256-thread summation played by one wavefront
# --------------------------------------------------------------------------- #
def test_status_ladder_on_whole_wave_rows(sa):
    """xtol chosen on the CPU with the oracle alone: the 16 deciding steps ||gbest_prev - gbest|| lie between 2.82e-4 and
    1.755e-3; 1.07e-3 sits in a central gap (9.83e-4 | 1.154e-3: 8.1 % and 7.9 % away), 9 runs end with status 0 and 7 with
    status 1, after 50 to 116 generations."""
    n, P, R = 130, 16, 16
    xtol = 1.07e-3
    x0 = np.random.RandomState(5).uniform(-1e-3, 1e-3, (R, P, n))
    lower, upper = box(n)
    opts = {"maxiter": 200, "ftol": 2e-5, "xtol": xtol}
    seeds = list(range(100, 100 + R))
    status, margin = [], []
    for r in range(R):  # the oracle alone
        best = []
        ref = oracle.minimize("sphere", np.stack([lower, upper], axis=1), x0=x0[r].copy(), method="pso", rng="philox",
                              options=dict(opts, popsize=P, seed=seeds[r], updating="deferred"),
                              callback=lambda X, res: best.append(np.array(res.x)))
        dx = np.linalg.norm(best[-2] - best[-1])
        assert ref.status == (0 if dx <= xtol else 1) and ref.fun <= opts["ftol"] and ref.nit < opts["maxiter"]
        status.append(ref.status)
        margin.append(abs(dx - xtol) / xtol)
    print("statuses", status, "smallest margin of dx to xtol %.4f" % min(margin))
    assert status.count(0) >= 4 and status.count(1) >= 4
    assert min(margin) > 0.02
    out = launch("sphere", lower, upper, P, seeds, x0=x0, **opts)
    check_oracle(out, "sphere", lower, upper, P, seeds, x0, opts)
    four = [status.index(0), R - 1 - status[::-1].index(0), status.index(1), R - 1 - status[::-1].index(1)]
    check_single(out, "sphere", lower, upper, P, seeds, x0, opts, runs=four)
    check_identities(sa, out, "sphere")
    # and the bottom rung: the same runs cut short end with -1 at maxiter
    cut = dict(opts, maxiter=2, ftol=1e-30)
    short = launch("sphere", lower, upper, P, seeds, x0=x0, **cut)
    assert (short[3] == -1).all() and (short[2] == 2).all()
    check_oracle(short, "sphere", lower, upper, P, seeds, x0, cut, runs=[0, R - 1])


# --------------------------------------------------------------------------- #
# ABI corners
# --------------------------------------------------------------------------- #
def test_shared_x0_same_start_different_runs(sa):
    n, P, R = 20, 12, 3
    x0 = np.random.RandomState(9).uniform(-5.12, 5.12, (P, n))
    keep = x0.copy()
    lower, upper = box(n)
    opts = {"maxiter": 6, "competitivity": 1.0}
    seeds = [5, 6, 7]
    shared = launch("rosenbrock", lower, upper, P, seeds, x0=x0, **opts)            # x0_stride = 0
    assert np.array_equal(x0, keep)
    check_oracle(shared, "rosenbrock", lower, upper, P, seeds, x0, opts)
    assert not np.array_equal(shared[4][0], shared[4][1]) and not np.array_equal(shared[4][1], shared[4][2])
    tiled = launch("rosenbrock", lower, upper, P, seeds, x0=np.tile(x0, (R, 1, 1)), **opts)  # x0_stride = P n
    assert identical(shared, tiled)


@pytest.mark.parametrize("n,P,R", [(3, 4, 300), (128, 40, 2)])
def test_same_launch_twice_same_bytes(sa, n, P, R):
    lower, upper = box(n)
    opts = {"maxiter": 10, "competitivity": 1.0}
    seeds = list(range(1000, 1000 + R))
    first = launch("rosenbrock", lower, upper, P, seeds, **opts)
    second = launch("rosenbrock", lower, upper, P, seeds, **opts)
    assert identical(first, second)
    check_oracle(first, "rosenbrock", lower, upper, P, seeds, None, opts, runs=sorted({0, R // 2, R - 1}))
    without = launch("rosenbrock", lower, upper, P, seeds, want_final=False, **opts)
    assert without[4] is None and identical(first[:4], without[:4])
