"""The ordered sweeps (csrc/sx_async.hip) for the tests: the table of whole-run edge cases that tests/test_gpu_immediate_edges.py
holds against the oracle (and tools/immediate_sensitivity.py checks on the oracle alone), and sx_de_async_generation driven
through the C ABI on host draws the test made up, next to the plain loop it must reproduce.  A plain helper module
(imported, not collected); nothing here touches the device at import."""

import ctypes as C

import numpy as np

from oracle.engine import DONORS, async_select, de_mutants
from oracle.objectives import OBJECTIVES

SEED = 11
RANGE = (-5.12, 5.12)
WIDE = "W"  # the longest row the sweeps serve, sx_wide_from() - 1: read from the library where the case runs (row_length)

# (method, objective, n, popsize, maxiter, extras).  What each group is there for:
#   n = 64 / 128 / 256 with the four hot objectives: the compile-time row length (NFIX) of both kernels;
#   ackley / griewank: 8 waves per workgroup, half the slots per round;
#   n = 512 / 1024: the run-time plan where the other kernels have a compile-time one (LONGSTATIC = 0);
#   n >= 1100 (DE) / 560 (PSO): fewer waves than the cap, more than 64 KiB of dynamic LDS; W: the fewest slots there are.
DE_CASES = [
    ("de", "ackley", 64, 70, 6, {"strategy": "best1bin"}),
    ("de", "rastrigin", 128, 70, 6, {"strategy": "rand1bin", "constraints": "Random", "mutation": 1.3}),
    ("de", "rastrigin", 256, 33, 5, {"strategy": "best2bin"}),
    ("de", "rosenbrock", 256, 33, 5, {"strategy": "best1bin"}),
    ("de", "sphere", 64, 130, 6, {"strategy": "rand2bin"}),
    ("de", "styblinski_tang", 64, 130, 6, {"strategy": "best2bin"}),
    ("de", "griewank", 130, 40, 6, {"strategy": "rand1bin", "constraints": "Random", "mutation": 1.3}),
    ("de", "quartic", 17, 70, 8, {"strategy": "rand2bin"}),
    ("de", "styblinski_tang", 300, 24, 5, {"strategy": "best1bin"}),
    ("de", "sphere", 512, 20, 4, {"strategy": "best1bin"}),
    ("de", "rosenbrock", 1024, 20, 4, {"strategy": "rand1bin"}),
    ("de", "ackley", 1500, 20, 3, {"strategy": "rand1bin"}),
    ("de", "griewank", WIDE, 12, 3, {"strategy": "best1bin"}),
    ("de", "quartic", WIDE, 12, 3, {"strategy": "rand2bin"}),
]
PSO_CASES = [
    ("pso", "ackley", 64, 70, 8, {}),
    ("pso", "rastrigin", 128, 40, 8, {}),
    ("pso", "ackley", 256, 33, 6, {}),
    ("pso", "rosenbrock", 64, 70, 8, {}),
    ("pso", "sphere", 128, 40, 8, {"constraints": "Shrink", "inertia": 0.91}),
    ("pso", "rosenbrock", 256, 33, 6, {}),
    ("pso", "griewank", 256, 33, 6, {}),
    ("pso", "quartic", 700, 20, 4, {}),
    ("pso", "sphere", 1024, 20, 4, {}),
    ("pso", "ackley", 1300, 20, 4, {}),
    ("pso", "griewank", WIDE, 12, 3, {}),
    ("cpso", "styblinski_tang", WIDE, 12, 4, {}),
    ("cpso", "ackley", 33, 96, 20, {}),
    ("pso", "rosenbrock", WIDE, 12, 3, {"constraints": "Shrink", "inertia": 0.95}),
]
# Shrink with an objective that is not + - * only: the oracle's own run is not bit-stable there, bounds instead of bits
# (rastrigin: 7 generations, not the 8 of its twin above -- with 8 the oracle's self-deviation came out at 1.05e-14 of the range,
#  past the 1e-14 a case may have here; with 7 it is 1.7e-15.  With popsize 33 it is 0.6: such a run proves nothing either way.)
SHRINK_CASES = [
    ("pso", "rastrigin", 128, 40, 7, {"constraints": "Shrink", "inertia": 0.91}),
    ("pso", "quartic", 700, 20, 4, {"constraints": "Shrink", "inertia": 0.95}),
    ("cpso", "ackley", 33, 96, 20, {"constraints": "Shrink", "inertia": 0.91}),
]
EDGE_CASES = DE_CASES + PSO_CASES + SHRINK_CASES


def case_id(case):
    method, objective, n, P, maxiter, extras = case
    words = [method, objective, str(n), str(P), str(maxiter)]
    words += [str(extras[k]) for k in ("strategy", "constraints", "mutation", "inertia") if k in extras]
    return "-".join(words)


def row_length(n):
    """The row length of a table entry: WIDE is read from the library (a host call, no device needed)."""
    if n != WIDE:
        return n
    from stochopy_amd import _lib

    return _lib.wide_from() - 1


def case_options(case):
    """(method, objective, bounds, options) of a table entry, as the oracle takes them."""
    method, objective, n, P, maxiter, extras = case
    n = row_length(n)
    opts = dict(extras, popsize=P, maxiter=maxiter, seed=SEED, updating="immediate", return_all=True)
    return method, objective, [list(RANGE)] * n, opts


# ---------------------------------------------------------------------------------------------------------------------------
# A DE sweep in which every individual depends on the one before it: donor t of individual i is individual i - 1 - t, every
# element takes the mutant.  Host draws (SX_RNG_HOST), so the test decides them.
# ---------------------------------------------------------------------------------------------------------------------------
CHAIN_F, CHAIN_CR, CHAIN_XTOL, CHAIN_FTOL, CHAIN_MAXITER = 0.3, 0.9, 1e-8, 1e-8, 10


def chain_inputs(P, n, strategy, seed=5):
    k = DONORS[strategy]
    i = np.arange(P)
    return dict(
        X=np.random.RandomState(seed).uniform(2.0, 4.0, (P, n)),
        donors=np.stack([(i - 1 - t) % P for t in range(k)]).astype(np.int32),
        r1=np.zeros((P, n)),
        irand=(i % n).astype(np.int32),
    )


def chain_reference(inp, strategy, generations):
    """de/_de.py:354-391 as a plain loop over i, on the crafted draws (the same ones in every generation).  Returns one dict
    per generation: X, fit, candfit, gbest, state (it, gfit, status, done) and `accepted`, the number of trials taken."""
    from stochopy_amd import _lib

    f = OBJECTIVES["sphere"]
    X = inp["X"].copy()
    P, n = X.shape
    fit = f(X)
    g = int(np.argmin(fit))
    gbest, gfit = X[g].copy(), fit[g]
    out, it = [], 1
    for _ in range(generations):
        it += 1
        candfit = np.empty(P)
        accepted = 0
        status = None
        for i in range(P):
            v = de_mutants(strategy, inp["donors"][:, i], CHAIN_F, X, gbest)
            take = inp["r1"][i] <= CHAIN_CR
            take[inp["irand"][i]] = True
            u = np.where(take, v, X[i])
            candfit[i] = f(u[None, :])[0]
            accepted += bool(candfit[i] <= fit[i])
            gbest, gfit, status = async_select(u, candfit[i], i, X, fit, gbest, gfit, CHAIN_XTOL, CHAIN_FTOL)
        if status is None and it >= CHAIN_MAXITER:
            status = -1
        out.append(dict(X=X.copy(), fit=fit.copy(), candfit=candfit, gbest=gbest.copy(), accepted=accepted,
                        state=(it, gfit, _lib.SX_STATUS_NONE if status is None else status, int(status is not None))))
    return out


def chain_sweeps(inp, strategy, generations):
    """The same generations through sx_de_async_generation, one launch each; the same list of dicts (without `accepted`)."""
    from stochopy_amd import _device, _lib

    X0 = inp["X"]
    P, n = X0.shape
    fit0 = OBJECTIVES["sphere"](X0)
    g = int(np.argmin(fit0))
    ctx = _device.Context()
    t = _device.torch()
    st = _lib.SxState(it=1, gbidx=g, gfit=fit0[g], dx=0.0, status=_lib.SX_STATUS_NONE, done=0)
    out = []
    with t.cuda.stream(ctx.stream):
        d_X, d_fit, d_gbest = ctx.upload(X0), ctx.upload(fit0), ctx.upload(X0[g])
        d_cand = ctx.upload(np.full(P, np.nan))
        d_state = ctx.upload(np.frombuffer(bytes(st), dtype=np.int64).copy())
        d_don, d_r1, d_irand = ctx.upload(inp["donors"]), ctx.upload(inp["r1"]), ctx.upload(inp["irand"])
        d_lower, d_upper = ctx.upload(np.full(n, -100.0)), ctx.upload(np.full(n, 100.0))
        d_rs = ctx.upload(np.full((P, n), np.nan))  # (constraints = 0: never read)
        a = _lib.SxDeArgs()
        a.buf0 = a.buf1 = d_X.data_ptr()
        a.fit, a.candfit, a.gbest, a.state = d_fit.data_ptr(), d_cand.data_ptr(), d_gbest.data_ptr(), d_state.data_ptr()
        a.lower, a.upper, a.resample = d_lower.data_ptr(), d_upper.data_ptr(), d_rs.data_ptr()
        a.donors, a.r1, a.irand = d_don.data_ptr(), d_r1.data_ptr(), d_irand.data_ptr()
        a.P, a.ld, a.row0, a.n = P, n, 0, n
        a.fun_id, a.strategy = _lib.FUN_IDS["sphere"], _lib.DE_STRATEGIES[strategy]
        a.constraints, a.rng, a.maxiter = 0, _lib.SX_RNG_HOST, CHAIN_MAXITER
        a.F, a.CR, a.xtol, a.ftol = CHAIN_F, CHAIN_CR, CHAIN_XTOL, CHAIN_FTOL
        for _ in range(generations):
            _lib.check(ctx.L.sx_de_async_generation(C.byref(a), ctx.stream_ptr), "sx_de_async_generation")
            s = ctx.read_state(d_state)
            out.append(dict(X=d_X.cpu().numpy(), fit=d_fit.cpu().numpy(), candfit=d_cand.cpu().numpy(),
                            gbest=d_gbest.cpu().numpy(), state=(int(s.it), float(s.gfit), int(s.status), int(s.done))))
    ctx.sync()
    return out
