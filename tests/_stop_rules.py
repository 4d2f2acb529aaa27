"""Stop-rule cases shared by the GPU test modules (imported, not collected): which seeds a case may be held to, decided by
the ORACLE ALONE, and the VD-CMA recipes that end on each rule the method can reach.

A seed is admitted if the oracle, with sigma nudged one ulp either way, keeps nit and status and moves fun by less than
1e-6 relative: only then is "nit, status and nfev exactly, fun to 1e-6" a bound a second implementation can keep
(tests/test_gpu_cma_runs_edges.py (d) has the finding that led to the rule)."""
import functools

import numpy as np

import oracle


def admitted(run, sigma, seeds):
    """run(seed, sigma) -> an oracle result.  [(seed, the oracle's run)] of the admitted seeds, and the table of all of them."""
    keep, table = [], []
    for seed in seeds:
        ref, lo, hi = (run(seed, s) for s in (sigma, np.nextafter(sigma, 0.0), np.nextafter(sigma, np.inf)))
        moved = max(abs(q.fun - ref.fun) / max(abs(ref.fun), 1e-300) for q in (lo, hi))
        ok = all((q.nit, q.status) == (ref.nit, ref.status) for q in (lo, hi)) and moved < 1e-6
        table.append("  seed %d oracle status %d nit %d | sigma - 1 ulp: %d %d | + 1 ulp: %d %d | fun moves %.2e | %s"
                     % (seed, ref.status, ref.nit, lo.status, lo.nit, hi.status, hi.nit, moved, "admitted" if ok else "no"))
        if ok:
            keep.append((seed, ref))
    return keep, table


# VD-CMA, popsize 10, maxiter 3000: rule -> (objective, half-width of the box, x0 per element or None, options).  ftol = -1
# turns rules 0 and 1 off.  Found in the oracle at n = 8 (seeds 700 ... 707: every one admitted, every one ends on the rule,
# after the generations given) and, where the run is short enough for a test, at n = 4097:
#   0   |xmean - xold| <= xtol with fbest < ftol                                    40 ... 48
#   1   fbest <= ftol                                                               85 ... 106
#  -3   any(0.2 sigma sd < 1e-10): a step size of 1e-10 ends generation 1           1
#  -5   the best values of the last `ilim` generations within 1e-10                 139 ... 158
#  -6   any(sigma sd > 1e3 insigma): a tiny step far from the minimum grows         23 ... 25 (445 at n = 4097)
#  -7   history and fitness within 1e-12: a tiny step at the sphere's minimum       3 (sigma = 1e-7: 3 ... 5 at n = 8, never at 4097)
#  -8   all(sigma |pc| < 1e-11 insigma) and sigma max(sd) < 1e-11 insigma           204 ... 240
# Rule -3 after many generations (rastrigin, n = 8, popsize 8 or 10: 189 ... 306) is not here: the oracle alone moves nit
# when sigma is nudged, for every seed of 700 ... 707 (tests/test_gpu_vd_runs.py holds status, fun and x of that case).
VD_RULES = {
    0: ("sphere", 3.0, None, dict(sigma=0.3, xtol=1.0, ftol=1e-3)),
    1: ("sphere", 3.0, None, dict(sigma=0.3)),
    -3: ("sphere", 3.0, None, dict(sigma=1e-10, ftol=-1.0)),
    -5: ("sphere", 3.0, None, dict(sigma=0.3, ftol=-1.0)),
    -6: ("sphere", 3.0, 2.9, dict(sigma=1e-6, ftol=-1.0)),
    -7: ("sphere", 3.0, 0.0, dict(sigma=1e-9, ftol=-1.0)),
    -8: ("styblinski_tang", 5.0, None, dict(sigma=1e5, ftol=-1.0)),
}
# the first wide row, n = 4097, where a generation of the oracle is 7 ms: the recipes that end within three generations;
# rules 0 and 1 with tolerances the first generation meets
VD_RULES_WIDE = {
    0: ("sphere", 3.0, None, dict(sigma=0.3, xtol=1e3, ftol=1e9)),
    1: ("sphere", 3.0, None, dict(sigma=0.3, ftol=1e9)),
    -3: VD_RULES[-3],
    -7: VD_RULES[-7],
}
VD_POPSIZE, VD_MAXITER, VD_TRIED = 10, 3000, tuple(range(700, 705))


def vd_case(rule, n):
    """(objective, bounds, x0, options) of the rule's recipe at n variables."""
    objective, half, x0, opts = (VD_RULES_WIDE if n > 4096 else VD_RULES)[rule]
    return objective, [[-half, half]] * n, None if x0 is None else np.full(n, x0), dict(opts, popsize=VD_POPSIZE, maxiter=VD_MAXITER)


@functools.lru_cache(maxsize=None)
def vd_admitted(rule, n):
    """The admitted seeds of VD_TRIED for (rule, n) with the oracle's runs (computed once, read-only), and the table.
    What every caller of this asks first: at least 4 seeds admitted, at least one of them ending on the rule."""
    objective, bounds, x0, opts = vd_case(rule, n)

    def run(seed, sigma):
        with np.errstate(all="ignore"):
            return oracle.minimize(objective, bounds, x0=x0, method="vdcma", rng="philox", options=dict(opts, seed=seed, sigma=sigma))

    keep, table = admitted(run, opts["sigma"], VD_TRIED)
    assert len(keep) >= 4 and any(ref.status == rule for _, ref in keep), "\n".join(table)
    return keep, table
