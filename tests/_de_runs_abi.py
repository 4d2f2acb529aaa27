"""The batched-runs DE kernel (csrc/sx_de_runs.hip) through its C ABI, with every output: optimize.minimize(runs=R) passes
xfinal = NULL and returns the best run's view; launch_runs fills _lib.SxDeRunsArgs exactly as optimize/_de.py
_minimize_runs does, but hands the kernel a real (R, P, n) xfinal buffer and returns all five outputs as numpy arrays.
A plain helper module for the GPU tests (imported, not collected)."""
import ctypes as C

import numpy as np


def stride_doubles(n, fused_above=256):
    """Doubles of LDS per population row, restated from the layout csrc/sx_de_runs.hip's header comment documents: the vector
    and 8 doubles of padding; rows whose objective terms are formed inside the reduction (more than `fused_above` elements)
    add the leaf sums [2][n // 64 + 2]."""
    return n + 8 if n <= fused_above else n + 8 + 2 * (n // 64 + 2)


def lds_bytes(P, n):
    """buf[2][P][stride] | fit[P] | 4 broadcast words, in bytes."""
    return 8 * (2 * P * stride_doubles(n) + P + 4)


def largest_popsize(lib, n):
    """The largest P with sx_de_runs_lds_bytes(P, n) > 0, by bisection (the function refuses everything above it)."""
    lo, hi = 2, 1 << 20
    assert lib.sx_de_runs_lds_bytes(lo, n) > 0 and lib.sx_de_runs_lds_bytes(hi, n) < 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if lib.sx_de_runs_lds_bytes(mid, n) > 0:
            lo = mid
        else:
            hi = mid
    return lo


def launch_runs(objective, lower, upper, P, seeds, x0=None, strategy="best1bin", constraints=None, maxiter=10, F=0.5, CR=0.9,
                xtol=1e-8, ftol=1e-8, want_final=True):
    """One sx_de_runs_launch of len(seeds) runs of `objective` (a factory name).  lower / upper: scalars or one value per
    dimension (then they give n; scalars need an x0 to give it).  x0: None, (P, n) shared by all runs (x0_stride = 0) or
    (R, P, n).  Returns xs (R, n), funs (R,), nits (R,), statuses (R,), xfinal (R, P, n) -- xfinal None if not wanted."""
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

    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        keys = np.array([_rng.philox_key(s) for s in seeds], dtype=np.uint32)
        d_keys = ctx.upload_async(keys.view(np.int32))
        d_bounds = ctx.upload_async(np.concatenate([lower, upper]))
        d_x0 = None if x0 is None else ctx.upload(x0)
        xs, funs = ctx.empty((R, n)), ctx.empty((R,))
        nits, statuses = ctx.empty((R,), dtype=t.int64), ctx.empty((R,), dtype=t.int32)
        # NaN-filled: an element the kernel does not write cannot pass for a value
        xfinal = t.full((R, P, n), float("nan"), dtype=t.float64, device=ctx.device) if want_final else None
        a = _lib.SxDeRunsArgs()
        a.keys, a.lower, a.upper = d_keys.data_ptr(), d_bounds[:n].data_ptr(), d_bounds[n:].data_ptr()
        a.x0 = None if d_x0 is None else d_x0.data_ptr()
        a.xs, a.funs, a.nits, a.statuses = xs.data_ptr(), funs.data_ptr(), nits.data_ptr(), statuses.data_ptr()
        a.xfinal = None if xfinal is None else xfinal.data_ptr()
        a.R, a.P, a.x0_stride = R, P, (P * n if d_x0 is not None and d_x0.dim() == 3 else 0)
        a.n, a.fun_id, a.strategy = n, _lib.FUN_IDS[objective], _lib.DE_STRATEGIES[strategy]
        a.constraints, a.maxiter = (1 if constraints == "Random" else 0), maxiter
        a.F, a.CR, a.xtol, a.ftol = F, CR, xtol, ftol
        _lib.check(ctx.L.sx_de_runs_launch(C.byref(a), ctx.stream_ptr), "sx_de_runs_launch")
        out = [xs.cpu().numpy(), funs.cpu().numpy(), nits.cpu().numpy(), statuses.cpu().numpy(),
               None if xfinal is None else xfinal.cpu().numpy()]
    return tuple(out)
