"""The batched-runs PSO / CPSO kernel (csrc/sx_pso_runs.hip) through its C ABI, with every output: optimize.minimize(runs=R)
passes xfinal = pbest_final = pbestfit_final = NULL and returns the best run's view; launch_runs fills _lib.SxPsoRunsArgs exactly
as optimize/_cpso.py _minimize_runs does, but hands the kernel real (R, P, n) / (R, P) buffers for the final swarm and returns
all seven outputs as numpy arrays.  A plain helper module for the tests (imported, not collected)."""
import ctypes as C

import numpy as np


def stride_doubles(n, fused_above=256):
    """Doubles of LDS per row of X, restated from the layout csrc/sx_pso_runs.hip's header comment documents: the vector and 8
    doubles of padding; rows whose objective terms are formed inside the reduction (more than `fused_above` elements) add the
    leaf sums [2][n // 64 + 2]."""
    return n + 8 if n <= fused_above else n + 8 + 2 * (n // 64 + 2)


LDS_LIMIT = 160 * 1024


def lds_bytes(P, n):
    """X[P][stride] | V[P][n] | pbest[P][n] | pbestfit[P] | gbest[n] | rad[P] | 4 broadcast words, in bytes, when that is
    within 160 KiB; else the same without V, which then lives in the workspace."""
    whole = 8 * (P * (stride_doubles(n) + 2 * n + 2) + n + 4)
    return whole if whole <= LDS_LIMIT else 8 * (P * (stride_doubles(n) + n + 2) + n + 4)


def workspace_bytes(R, P, n):
    """0 when V is in the LDS, else R (P, n) arrays of doubles."""
    return 0 if 8 * (P * (stride_doubles(n) + 2 * n + 2) + n + 4) <= LDS_LIMIT else 8 * R * P * n


def largest_popsize(lib, n):
    """The largest P with sx_pso_runs_lds_bytes(P, n) > 0, by bisection (the function refuses everything above it)."""
    lo, hi = 2, 1 << 20
    assert lib.sx_pso_runs_lds_bytes(lo, n) > 0 and lib.sx_pso_runs_lds_bytes(hi, n) < 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.sx_pso_runs_lds_bytes(mid, n) > 0:
            lo = mid
        else:
            hi = mid
    return lo


def restart_delta(P, maxiter):
    """cpso/_cpso.py:215-216."""
    return float(np.log(1.0 + 0.003 * P) / np.max((0.2, np.log(0.01 * maxiter))))


def launch_runs(objective, lower, upper, P, seeds, x0=None, constraints=None, maxiter=10, inertia=0.7298, cognitivity=1.49618,
                sociability=1.49618, competitivity=None, xtol=1e-8, ftol=1e-8, want_final=True):
    """One sx_pso_runs_launch of len(seeds) runs of `objective` (a factory name).  lower / upper: scalars or one value per
    dimension (then they give n; scalars need an x0 to give it).  x0: None, (P, n) shared by all runs (x0_stride = 0) or
    (R, P, n).  Returns xs (R, n), funs (R,), nits (R,), statuses (R,), xfinal (R, P, n), pbest (R, P, n), pbestfit (R, P)
    -- the last three None if not wanted."""
    from stochopy_amd import _device, _lib, _rng

    seeds = [int(s) for s in seeds]
    R = len(seeds)
    if x0 is not None:
        x0 = np.array(x0, dtype=np.float64)
        n = x0.shape[-1]
        assert x0.shape in ((P, n), (R, P, n))
    else:
        n = max(np.size(lower), np.size(upper))
    lower = np.ascontiguousarray(np.broadcast_to(np.asarray(lower, dtype=np.float64), (n,)))
    upper = np.ascontiguousarray(np.broadcast_to(np.asarray(upper, dtype=np.float64), (n,)))
    gamma = float(competitivity) if competitivity else 0.0

    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        keys = np.array([_rng.philox_key(s) for s in seeds], dtype=np.uint32)
        d_keys = ctx.upload_async(keys.view(np.int32))
        d_bounds = ctx.upload_async(np.concatenate([lower, upper]))
        d_x0 = None if x0 is None else ctx.upload(x0)
        xs, funs = ctx.empty((R, n)), ctx.empty((R,))
        nits, statuses = ctx.empty((R,), dtype=t.int64), ctx.empty((R,), dtype=t.int32)
        # filled with a value no run produces: an element the kernel does not write cannot pass for a result
        fill = -12345.678
        finals = [t.full(shape, fill, dtype=t.float64, device=ctx.device) if want_final else None
                  for shape in ((R, P, n), (R, P, n), (R, P))]
        a = _lib.SxPsoRunsArgs()
        a.keys, a.lower, a.upper = d_keys.data_ptr(), d_bounds[:n].data_ptr(), d_bounds[n:].data_ptr()
        a.x0 = None if d_x0 is None else d_x0.data_ptr()
        a.xs, a.funs, a.nits, a.statuses = xs.data_ptr(), funs.data_ptr(), nits.data_ptr(), statuses.data_ptr()
        a.xfinal, a.pbest_final, a.pbestfit_final = [None if f is None else f.data_ptr() for f in finals]
        vwork = int(ctx.L.sx_pso_runs_workspace_bytes(R, P, n))
        assert vwork == workspace_bytes(R, P, n)
        d_vwork = ctx.empty((vwork // 8,)) if vwork else None
        a.vwork = None if d_vwork is None else d_vwork.data_ptr()
        a.R, a.P, a.x0_stride = R, P, (P * n if d_x0 is not None and d_x0.dim() == 3 else 0)
        a.n, a.fun_id = n, _lib.FUN_IDS[objective]
        a.constraints, a.maxiter = (1 if constraints == "Shrink" else 0), maxiter
        a.w, a.c1, a.c2, a.gamma = inertia, cognitivity, sociability, gamma
        a.delta = restart_delta(P, maxiter) if gamma else 0.0
        a.xtol, a.ftol = xtol, ftol
        _lib.check(ctx.L.sx_pso_runs_launch(C.byref(a), ctx.stream_ptr), "sx_pso_runs_launch")
        out = [xs.cpu().numpy(), funs.cpu().numpy(), nits.cpu().numpy(), statuses.cpu().numpy()]
        out += [None if f is None else f.cpu().numpy() for f in finals]
    if want_final:
        assert not (out[4] == fill).any() and not (out[5] == fill).any() and not (out[6] == fill).any()
    return tuple(out)
