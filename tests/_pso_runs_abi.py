"""The batched-runs PSO / CPSO kernel (csrc/sx_pso_runs.hip) with every output: optimize.minimize(runs=R) passes xfinal =
pbest_final = pbestfit_final = NULL and returns the best run's view; launch_runs builds the batch minimize() launches
(optimize/_cpso.py _runs_batch) with real (R, P, n) / (R, P) buffers for the final swarm and returns all seven outputs as numpy
arrays.  A plain helper module for the tests (imported, not collected)."""
import numpy as np

from _runs_abi import FILL, largest, launch_filled


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
    """The largest P with sx_pso_runs_lds_bytes(P, n) > 0 (the function refuses everything above it)."""
    return largest(lambda p: lib.sx_pso_runs_lds_bytes(p, n) > 0, 2, 1 << 20)


FINALS = ("xfinal", "pbest_final", "pbestfit_final")


def launch_runs(objective, lower, upper, P, seeds, x0=None, constraints=None, maxiter=10, inertia=0.7298, cognitivity=1.49618,
                sociability=1.49618, competitivity=None, xtol=1e-8, ftol=1e-8, want_final=True):
    """One sx_pso_runs_launch of len(seeds) runs of `objective` (a factory name).  lower / upper: scalars or one value per
    dimension (then they give n; scalars need an x0 to give it).  x0: None, (P, n) shared by all runs (x0_stride = 0) or
    (R, P, n).  Returns xs (R, n), funs (R,), nits (R,), statuses (R,), xfinal (R, P, n), pbest (R, P, n), pbestfit (R, P)
    -- the last three None if not wanted."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize._cpso import _runs_batch

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
    batch = _runs_batch(seeds, _lib.FUN_IDS[objective], lower, upper, x0, maxiter, P, inertia, cognitivity, sociability,
                        competitivity, constraints, xtol, ftol, outputs=FINALS if want_final else ())
    vwork = batch.dev.get("vwork")
    assert (0 if vwork is None else 8 * vwork.numel()) == workspace_bytes(R, P, n)
    out = launch_filled(batch, dict.fromkeys(FINALS, FILL) if want_final else {})
    if want_final:
        assert not (out["xfinal"] == FILL).any() and not (out["pbest_final"] == FILL).any()
        assert not (out["pbestfit_final"] == FILL).any()
    return (out["xs"], out["funs"], out["nits"], out["statuses"]) + tuple(out.get(k) for k in FINALS)
