"""The batched-runs DE kernel (csrc/sx_de_runs.hip) with every output: optimize.minimize(runs=R) passes xfinal = NULL and
returns the best run's view; launch_runs builds the batch minimize() launches (optimize/_de.py _runs_batch) with a real
(R, P, n) xfinal buffer and returns all five outputs as numpy arrays.  A plain helper module for the GPU tests (imported,
not collected)."""
import numpy as np

from _runs_abi import largest, launch_filled


def stride_doubles(n, fused_above=256):
    """Doubles of LDS per population row, restated from the layout csrc/sx_de_runs.hip's header comment documents: the vector
    and 8 doubles of padding; rows whose objective terms are formed inside the reduction (more than `fused_above` elements)
    add the leaf sums [2][n // 64 + 2]."""
    return n + 8 if n <= fused_above else n + 8 + 2 * (n // 64 + 2)


def lds_bytes(P, n):
    """buf[2][P][stride] | fit[P] | 4 broadcast words, in bytes."""
    return 8 * (2 * P * stride_doubles(n) + P + 4)


def largest_popsize(lib, n):
    """The largest P with sx_de_runs_lds_bytes(P, n) > 0 (the function refuses everything above it)."""
    return largest(lambda p: lib.sx_de_runs_lds_bytes(p, n) > 0, 2, 1 << 20)


def launch_runs(objective, lower, upper, P, seeds, x0=None, strategy="best1bin", constraints=None, maxiter=10, F=0.5, CR=0.9,
                xtol=1e-8, ftol=1e-8, want_final=True):
    """One sx_de_runs_launch of len(seeds) runs of `objective` (a factory name).  lower / upper: scalars or one value per
    dimension (then they give n; scalars need an x0 to give it).  x0: None, (P, n) shared by all runs (x0_stride = 0) or
    (R, P, n).  Returns xs (R, n), funs (R,), nits (R,), statuses (R,), xfinal (R, P, n) -- xfinal None if not wanted."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize._de import _runs_batch

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
    batch = _runs_batch(seeds, _lib.FUN_IDS[objective], lower, upper, x0, maxiter, P, F, CR, strategy, constraints, xtol, ftol,
                        outputs=("xfinal",) if want_final else ())
    # NaN-filled: an element the kernel does not write cannot pass for a value
    out = launch_filled(batch, {"xfinal": float("nan")} if want_final else {})
    return out["xs"], out["funs"], out["nits"], out["statuses"], out.get("xfinal")
