"""The batched-runs CMA-ES kernel (csrc/sx_cma_runs.hip) at its LDS limits, on every stop rule it can be brought to, and
generation by generation, through its C ABI with real nfevs / sigmas / xmeans buffers (tests/_cma_runs_abi.py launch_runs).

(a), (b)  GENERATION 1 against a plain reference (_cma_runs_abi.generation_one: numpy, stable argsort, long-double sums; held to
    the oracle's probe on the CPU in tests/test_cma_runs_host.py).  A run with maxiter = 1 is one generation from C = B = I, D = 1:
    arx = xmean0 + sigma z, xmean = w @ arx[order[:mu]], x = arx[order[0]] xstd + xm.  sigma is 2^-10, so sigma z is exact and
    arx is ONE rounding whether or not the device contracts it to an fma.  Bounds:
      nit, nfev, status   exact;
      x                   2 ulp per element, the ulp of |arx xstd| + |xm|: the magnitude the one multiply-add works at (the
                          product's rounding, which a contraction to fma drops, and the sum's; the boxes of (a) keep both terms
                          of one sign, so this is the ulp of x itself within a factor 2) -- this pins the best ROW;
      xmean               mu 2^-53 sum_k |w_k arx_k| per element: a sum of mu terms in index order, contracted or not;
      sigma, fun          rtol 1e-6, the project's `fun` tolerance (the device's objective and exp are not the host's).
    What these bounds do NOT budget for is the few ulp by which the device's log / sincos differ from libm's in z
    (tests/test_gpu_cmaes.py::test_philox_normals_vs_oracle).  They reach a candidate scaled by sigma |z| / |arx| -- 2^-10 here,
    with standardised means of 0.1 ... 0.9 -- and flip its last bit about once in a thousand elements; only mu = 1 (P = 2) has a
    bound below one ulp of arx, over 16 elements.
    Shapes: P at the LDS limit of n = 1, 16, 17, 32, each side of 64 KiB (where sx_cma_runs_launch raises the kernel's
    dynamic-LDS attribute) and each side of the cross-over at which the candidates outgrow the Jacobi storage they share the
    region U with; a per-dimension, asymmetric box (no centre is 0), a starting point per run.  rosenbrock at n = 1 is an empty
    sum: every row ties at 0.0.
(b) Tied +inf fitness: sphere on [-5e154, 5e154]^n makes every row +inf (the ranking is then the index order), rosenbrock on
    [-5e76, 5e76]^3 mixes +inf and finite rows.  A seed is admitted only if no term of any candidate lies within a factor 4 of
    the overflow threshold (host and device then classify the same rows), and a mixed seed only if mu exceeds the number of
    finite rows.  All-inf: the starting points are placed at 0.6 ... 0.95 of the half-width, every seed is admitted.  Mixed: a
    row is +inf iff |arx_i| > 0.73 for some i < n - 1 and the factor 4 forbids 0.52 ... 1.03, so the rows of one run -- a
    unimodal sample around one mean -- would have to straddle a gap of half a unit without one element of P (n - 1) falling into
    it.  Searched on the CPU: seeds 700 ... 763, sigma 0.1, 0.5, 2, 8, P = 12, 65, 130 (n = 3) and 432 (n = 32): the seeds of
    MIXED below at P = 12 (one row of 12 finite, mu = 6) and none at P = 65, 130, 432 -- those three sizes are run all-inf only.
(c) The first six generations against the oracle's probe: a launch with maxiter = g ends at generation g with status -1 and
    shows that generation's xmean and sigma.  rtol 1e-5 / atol 1e-7 and rtol 1e-6, the tolerances `x` and `fun` are held to.
(d) Every stop rule but -3 (tests/test_gpu_cma_runs.py reaches -1, 1, -5, -2): 0, -4, -6, -7, -8, with ftol = -1 where rules 0
    and 1 must be off, maxiter 3000, seeds 700 ... 707 tried per rule (700 ... 711 for rule -4).
    A seed is admitted by the ORACLE ALONE: nudged one ulp in
    sigma either way it keeps nit and status and moves fun by less than 1e-6 relative; the admitted seeds run in one launch and
    every one of them is held to the oracle (nit, nfev, status exactly, fun rtol 1e-6, x rtol 1e-5 / atol 1e-7).
    Rule -8: with the sphere at sigma = 1e5 no seed of 700 ... 715 is admitted (fun, a rounding-sized number, moves by 8e-6 ...
    1e-3); styblinski_tang, whose minimum is -78, admits all 16.  Rule -4: the sphere on [[-1e-4, 1e-4], [-1e4, 1e4]] with
    sigma = 0.3 ends with -4 for seed 707 alone of 700 ... 763 (63 of the 64 are admitted, the others end with -2; the case is
    kept with its first 8 seeds); with sigma = 1 it ends with -4 for 700, 703, 707 and 711, all admitted.
    A FINDING, and why that recipe is not here: rosenbrock on [[-1e5, 1e5], [-1, 1]] with sigma = 1e5 ends with -4 for 12 seeds
    of 700 ... 715, 10 of them admitted.  On the device, of the admitted seeds 701, 702, 704, 705, 706, 707: fun of 701 and 706
    was 1.76e-6 and 1.13e-6 off (the oracle alone moved it by 2.7e-7 and 3.0e-8), and 704 (status -2) stopped at generation 116,
    not 114.  No kernel fault: those runs stop FAR from their minimum (fun 1e9, x = (-108, 8178)) while rule -2's quantity is 3 %
    under its threshold (9.70e-11 against 1e-10 at generation 114 of seed 704), and in every case of this file the device is
    10 ... 40 times further from the oracle than the oracle is from itself under a one-ulp nudge (it differs in thousands of
    roundings, not one): with 2.7e-7 for one ulp, rtol 1e-6 is not a bound the run can keep.  An eigensolver with relatively
    accurate eigenvalues in the oracle's place (2 x 2, closed form in long double) moved none of them by more than 8e-8.
    Rule -3 (TolXUp ... `0.2 sigma sqrt(C_ii) < 1e-10` for one i, after rule -2 has looked at ONE axis) has no test.  Searched in
    the CPU oracle, ftol = -1, maxiter 3000, popsize 10: all seven objectives, n = 2, 3, 5, 8, the boxes [-3, 3]^n, one
    dimension 1e5 times wider or narrower than the others (first or last), a ramp of half-widths 10^-2.5 ... 10^2.5; sigma
    1e-9, 1e-6, 1e-3, 0.3, 1e2, 1e5; then griewank with one dimension 1e2 ... 1e5 times wider, n = 2 ... 8, sigma 0.1 ... 3.
    2 of 1680 and 9 of 1152 runs end with -3, all after 379 ... 1231 generations.  The best recipe (griewank, n = 5, last dimension
    [-1e5, 1e5], sigma 0.3) reaches -3 for seeds 700 and 702 of 700 ... 763, and 702 alone is admitted: no recipe has 4
    admitted seeds among 16.
(e) mu = 1 and mu = P, whole runs, the seeds admitted as in (d) (from 5 on).  (sphere, 3, 10) with mu = 1 has mu + 1 < n: C is
    the identity plus a rank-2 update, one eigenvalue is repeated, and no two eigensolvers agree on a basis of its eigenspace
    (tests/test_gpu_cmaes.py _eigenbasis_is_determined).  The oracle alone changes nit for 7 of the seeds 5 ... 12 when sigma is
    nudged by one ulp (60 | 60 | 56, 59 | 61 | 52, ...) and NONE of 5 ... 20 is admitted; on the device the eight runs of 5 ... 12
    ended with status 1 after 53, 59, 56, 61, 55, 52, 56, 56 generations against the oracle's 60, 59, 62, 61, 53, 54, 57, 52.
    That case is therefore not run; (sphere, 2, 10) is the mu = 1 case whose basis is determined.
(f) whole runs at the LDS limits, twice (same bytes), then a small shape of the same kernel
    instantiation (the raised attribute is sticky; M2 = 32 has no shape below 41 KiB, so "small" is under 64 KiB), (g) 1100
    workgroups.  The figures the tests print are in profiles/cma_runs_edges_gpu_tests.txt."""
import functools
import os
import sys
import types

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cma_runs_abi as abi  # noqa: E402
import _stop_rules  # noqa: E402
from test_gpu_cma_runs import _same_run  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("xs", "funs", "nits", "statuses", "nfevs", "sigmas", "xmeans")
_ID = lambda c: "_".join(str(v) for v in c[:3])  # noqa: E731


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(scope="module")
def lib(sa):
    from stochopy_amd import _lib

    return _lib.lib()


def launch(objective, lower, upper, P, seeds, **kw):
    return types.SimpleNamespace(**dict(zip(NAMES, abi.launch_runs(objective, lower, upper, P, seeds, **kw))))


def bits(res):
    return tuple(getattr(res, k).tobytes() for k in NAMES)


def box(n, lo=-3.0, hi=3.0):
    return np.full(n, lo), np.full(n, hi)


def oracle_run(objective, lower, upper, P, seed, x0=None, probe=None, **opts):
    with np.errstate(all="ignore"):
        return oracle.minimize(objective, np.transpose([lower, upper]), x0=x0, method="cmaes", rng="philox",
                               options=dict(opts, popsize=P, seed=seed, eigh="canonical", probe=probe))


def test_the_launcher_is_the_front_end(sa):
    """launch_runs adds no behaviour: the bytes of optimize.minimize(runs=R) on one shape."""
    n, P, R, seed = 5, 12, 8, 40
    lower, upper = abi.gen1_box(n)
    opts = dict(maxiter=40, sigma=0.2, muperc=0.5, xtol=1e-8, ftol=1e-8)
    res = sa.optimize.minimize(sa.factory.rosenbrock, np.transpose([lower, upper]).tolist(), method="cmaes",
                               options=dict(opts, popsize=P, runs=R, seed=seed, backend="hip", rng="philox"))
    got = launch("rosenbrock", lower, upper, P, range(seed, seed + R), **opts)
    for k in ("xs", "funs", "nits", "statuses", "sigmas"):
        assert getattr(got, k).dtype == getattr(res, k).dtype and getattr(got, k).tobytes() == getattr(res, k).tobytes(), k
    assert (got.nfevs == got.nits * P).all() and got.nfevs.dtype == np.int64


# ---- (a), (b): generation 1
def check_generation_one(tag, objective, lower, upper, P, seeds, x0, sigma):
    R, n = len(seeds), len(lower)
    got = launch(objective, lower, upper, P, seeds, x0=x0, maxiter=1, sigma=sigma)
    refs = [abi.generation_one(objective, lower, upper, P, s, None if x0 is None else x0[r], sigma=sigma)
            for r, s in enumerate(seeds)]
    worst = dict(x_ulp=0.0, xmean_of_bound=0.0, sigma_rel=0.0, fun_rel=0.0)
    for r, ref in enumerate(refs):
        worst["x_ulp"] = max(worst["x_ulp"], float((np.abs(got.xs[r] - ref["x"]) / np.spacing(ref["xparts"])).max()))
        bound = ref["mu"] * 2.0 ** -53 * ref["absum"]
        worst["xmean_of_bound"] = max(worst["xmean_of_bound"], float((np.abs(got.xmeans[r] - ref["xmean"]) / bound).max()))
        worst["sigma_rel"] = max(worst["sigma_rel"], abs(got.sigmas[r] - ref["sigma"]) / ref["sigma"])
        if np.isfinite(ref["fun"]) and ref["fun"] != 0.0:
            worst["fun_rel"] = max(worst["fun_rel"], abs(got.funs[r] - ref["fun"]) / abs(ref["fun"]))
    print("gen1 %s %s n %d P %d R %d lds %d mu %d:" % (tag, objective, n, P, R, abi.lds_bytes(P, n), refs[0]["mu"]),
          " ".join("%s %.3g" % kv for kv in worst.items()))
    assert (got.nits == 1).all() and (got.nfevs == P).all() and (got.statuses == -1).all()
    for r, ref in enumerate(refs):
        assert (np.abs(got.xs[r] - ref["x"]) <= 2.0 * np.spacing(ref["xparts"])).all(), (r, got.xs[r], ref["x"])
        assert (np.abs(got.xmeans[r] - ref["xmean"]) <= ref["mu"] * 2.0 ** -53 * ref["absum"]).all(), (r, got.xmeans[r], ref["xmean"])
        assert np.isclose(got.sigmas[r], ref["sigma"], rtol=1e-6, atol=0.0), (r, got.sigmas[r], ref["sigma"])
        assert np.isclose(got.funs[r], ref["fun"], rtol=1e-6, atol=1e-300), (r, got.funs[r], ref["fun"])
    return refs


def test_generation_one_shapes_are_the_librarys_limits(lib):
    assert abi.gen1_shapes(lib) == abi.GEN1_LITERALS
    for n, P in abi.GEN1_LITERALS:
        assert lib.sx_cma_runs_lds_bytes(P, n) == abi.lds_bytes(P, n)
    for n in (16, 32):
        k = abi.largest_popsize_below(64 * 1024, n)
        assert (n, k) in abi.GEN1_LITERALS and abi.lds_bytes(k, n) <= 64 * 1024 < abi.lds_bytes(k + 1, n)
    for n in (16, 17, 32):
        x = abi.crossover_popsize(n)
        assert x * (n + 8) <= abi.jacobi_doubles(n) < (x + 1) * (n + 8)
        assert abi.lds_bytes(x + 2, n) - abi.lds_bytes(x + 1, n) >= 8 * (n + 8)  # (the candidates are the larger tenant)


@pytest.mark.parametrize("objective", ["sphere", "rosenbrock"])
@pytest.mark.parametrize("shape", abi.GEN1_LITERALS, ids=lambda s: "n%d_p%d" % s)
def test_generation_one_against_the_plain_reference(sa, shape, objective):
    n, P = shape
    R = 16 if P < 100 else (8 if P < 400 else 4)
    lower, upper = abi.gen1_box(n)
    check_generation_one("a", objective, lower, upper, P, [700 + r for r in range(R)], abi.gen1_x0(n, R), abi.GEN1_SIGMA)


FMAX = np.longdouble(np.finfo(np.float64).max)


def terms_clear_of_overflow(objective, X):
    """No term of any row of X (un-standardised candidates) within a factor 4 of the overflow threshold."""
    X = X.astype(np.longdouble)
    if objective == "sphere":
        t = X * X
    else:  # rosenbrock
        t = np.concatenate([100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2, (1.0 - X[:, :-1]) ** 2], axis=1)
    return not ((t >= FMAX / 4.0) & (t <= FMAX * 4.0)).any()


@pytest.mark.parametrize("shape", [(3, 12), (3, 65), (3, 130), (32, 432)], ids=lambda s: "n%d_p%d" % s)
def test_ranking_when_every_row_is_inf(sa, shape):
    n, P = shape
    R = 4
    lower, upper = box(n, -5e154, 5e154)
    r, i = np.arange(R)[:, None], np.arange(n)[None, :]
    x0 = np.where((r + i) % 2 == 0, 1.0, -1.0) * (0.6 + 0.35 * ((5 * r + 3 * i) % 8) / 7.0) * 5e154
    seeds = [700 + k for k in range(R)]
    refs = check_generation_one("b all-inf", "sphere", lower, upper, P, seeds, x0, abi.GEN1_SIGMA)
    for ref in refs:  # (what the case is there for, and its admission)
        assert np.isposinf(ref["fit"]).all() and (ref["order"] == np.arange(P)).all()
        assert np.isfinite(ref["arx"]).all() and terms_clear_of_overflow("sphere", ref["arx"] * 5e154)


# (sigma, seed) admitted at n = 3, P = 12 by the search the module docstring describes
MIXED = [(2.0, 703), (8.0, 706)]


@pytest.mark.parametrize("cfg", MIXED, ids=lambda c: "sigma%g_seed%d" % c)
def test_ranking_when_inf_and_finite_rows_mix(sa, cfg):
    sigma, seed = cfg
    n, P = 3, 12
    lower, upper = box(n, -5e76, 5e76)
    ref, = check_generation_one("b mixed", "rosenbrock", lower, upper, P, [seed], None, sigma)  # (a launch of one run)
    finite = int(np.isfinite(ref["fit"]).sum())
    print("  mixed: %d of %d rows +inf, mu %d" % (P - finite, P, ref["mu"]))
    assert 0 < finite < ref["mu"] and np.isposinf(ref["fit"][~np.isfinite(ref["fit"])]).all()  # tie order decides xmean
    assert terms_clear_of_overflow("rosenbrock", ref["arx"] * 5e76)


# ---- (c): the first generations against the oracle's probe
@functools.lru_cache(maxsize=None)
def probed(objective, n, P, seed, sigma, gens):
    """after[...] of generations 1 ... gens of one oracle run (computed once, read-only)."""
    seen = []
    lower, upper = abi.gen1_box(n)
    oracle_run(objective, lower, upper, P, seed, maxiter=gens, sigma=sigma, probe=lambda it, before, after: seen.append(after))
    assert len(seen) == gens
    return seen


@pytest.mark.parametrize("cfg", [("rosenbrock", 5, 12), ("rastrigin", 32, 64), ("sphere", 17, 172), ("sphere", 32, 432)], ids=_ID)
def test_first_generations_against_the_oracle_probe(sa, cfg):
    objective, n, P = cfg
    R, sigma, gens = 4, 0.3, 6
    seeds = [700 + r for r in range(R)]
    lower, upper = abi.gen1_box(n)
    failures = []
    for g in range(1, gens + 1):
        got = launch(objective, lower, upper, P, seeds, maxiter=g, sigma=sigma)
        assert (got.nits == g).all() and (got.nfevs == g * P).all() and (got.statuses == -1).all()
        dx = ds = 0.0
        for r, seed in enumerate(seeds):
            after = probed(objective, n, P, seed, sigma, gens)[g - 1]
            dx = max(dx, float(np.abs(got.xmeans[r] - after["xmean"]).max()))
            ds = max(ds, abs(got.sigmas[r] - after["sigma"]) / after["sigma"])
            if not (np.allclose(got.xmeans[r], after["xmean"], rtol=1e-5, atol=1e-7)
                    and np.isclose(got.sigmas[r], after["sigma"], rtol=1e-6, atol=0.0)):
                failures.append((g, r))
        print("gens %s n %d P %d generation %d: max |xmean - oracle| %.3g, max rel sigma %.3g" % (objective, n, P, g, dx, ds))
    assert not failures, failures


# ---- (d): every stop rule
TRIED = list(range(700, 708))
SPHERE_1E8 = (np.array([-1e-4, -1e4]), np.array([1e-4, 1e4]))
# name: (rule, at least so many admitted seeds end with it, objective, lower, upper, x0, options, seeds tried)
RULES = {
    "rule0_sphere_n3": (0, 4, "sphere", *box(3), None, dict(sigma=0.3, xtol=1.0, ftol=1e-3), TRIED),
    "rule-6_sphere_n2": (-6, 4, "sphere", *box(2), 2.9, dict(sigma=1e-6, ftol=-1.0), TRIED),
    "rule-6_sphere_n4": (-6, 4, "sphere", *box(4), 2.9, dict(sigma=1e-6, ftol=-1.0), TRIED),
    "rule-7_sphere_n2": (-7, 4, "sphere", *box(2), 0.0, dict(sigma=1e-7, ftol=-1.0), TRIED),
    "rule-8_styblinski_tang_n2": (-8, 4, "styblinski_tang", *box(2, -5.0, 5.0), None, dict(sigma=1e5, ftol=-1.0), TRIED),
    "rule-4_sphere_n2_sigma1": (-4, 4, "sphere", *SPHERE_1E8, None, dict(sigma=1.0, ftol=-1.0), list(range(700, 712))),
    "rule-4_sphere_n2_sigma0.3": (-4, 1, "sphere", *SPHERE_1E8, None, dict(sigma=0.3, ftol=-1.0), TRIED),
}


def admitted(objective, lower, upper, P, x0, opts, seeds, maxiter=3000):
    """[(seed, the oracle's run)] of the seeds the oracle ALONE is insensitive for, and the table of all of them."""
    return _stop_rules.admitted(lambda seed, s: oracle_run(objective, lower, upper, P, seed, x0=x0, maxiter=maxiter, **dict(opts, sigma=s)),
                                opts["sigma"], seeds)


@pytest.mark.parametrize("name", sorted(RULES))
def test_every_stop_rule_against_the_oracle(sa, name):
    rule, least, objective, lower, upper, x0, opts, tried = RULES[name]
    n, P = len(lower), 10
    x0 = None if x0 is None else np.full(n, x0)
    keep, table = admitted(objective, lower, upper, P, x0, opts, tried)
    print(name, opts)
    print("\n".join(table))
    assert len(keep) >= 4 and sum(ref.status == rule for _, ref in keep) >= least
    got = launch(objective, lower, upper, P, [s for s, _ in keep], x0=x0, maxiter=3000, **opts)
    print("  device nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    print("  rel fun", ["%.3g" % (abs(got.funs[r] - ref.fun) / max(abs(ref.fun), 1e-300)) for r, (_, ref) in enumerate(keep)])
    for r, (_, ref) in enumerate(keep):
        _same_run(got, r, ref, P)
        assert got.nfevs[r] == ref.nfev


# ---- (e): mu at both ends; (objective, n, P, muperc, maxiter, sigma, seeds tried)
@pytest.mark.parametrize("cfg", [("sphere", 2, 10, 0.1, 100, 0.1, 8), ("sphere", 3, 10, 1.0, 100, 0.1, 8),
                                 ("rosenbrock", 20, 48, 1.0, 60, 0.2, 8)],
                         ids=lambda c: "%s_n%d_p%d_muperc%g" % c[:4])
def test_mu_at_both_ends(sa, cfg):
    objective, n, P, muperc, maxiter, sigma, tried = cfg
    lower, upper = box(n)
    opts = dict(sigma=sigma, muperc=muperc)
    keep, table = admitted(objective, lower, upper, P, None, opts, range(5, 5 + tried), maxiter=maxiter)
    print(cfg, "mu", int(muperc * P))
    print("\n".join(table))
    assert int(muperc * P) in (1, P) and len(keep) >= 4
    got = launch(objective, lower, upper, P, [s for s, _ in keep], maxiter=maxiter, **opts)
    print("  device nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    for r, (_, ref) in enumerate(keep):
        _same_run(got, r, ref, P)


# ---- (f): whole runs at the LDS limits; (objective, n, its small shape of the same kernel instantiation <objective, M2>)
@pytest.mark.parametrize("cfg", [("rastrigin", 32, (32, 64)), ("sphere", 17, (17, 34)), ("sphere", 1, (6, 12)),
                                 ("rosenbrock", 16, (12, 130))], ids=lambda c: "%s_n%d" % c[:2])
def test_whole_runs_at_the_lds_limit(sa, lib, cfg):
    objective, n, small = cfg
    P = abi.largest_popsize(lib, n)
    assert (n, P) in abi.GEN1_LITERALS and abi.lds_bytes(P, n) > 64 * 1024
    R, maxiter, sigma = 4, 12, 0.3
    seeds = [900 + r for r in range(R)]
    lower, upper = box(n)
    got = launch(objective, lower, upper, P, seeds, maxiter=maxiter, sigma=sigma)
    again = launch(objective, lower, upper, P, seeds, maxiter=maxiter, sigma=sigma)
    assert bits(got) == bits(again)
    print(cfg, "P", P, "lds", abi.lds_bytes(P, n), "nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    for r, seed in enumerate(seeds):
        _same_run(got, r, oracle_run(objective, lower, upper, P, seed, maxiter=maxiter, sigma=sigma), P)
    # the attribute the large launch raised stays on the kernel: a small shape of the same instantiation is still served
    n2, P2 = small
    assert abi.solver_size(n2) == abi.solver_size(n) and abi.lds_bytes(P2, n2) < 64 * 1024
    lower, upper = box(n2)
    got = launch(objective, lower, upper, P2, seeds, maxiter=maxiter, sigma=sigma)
    for r, seed in enumerate(seeds):
        _same_run(got, r, oracle_run(objective, lower, upper, P2, seed, maxiter=maxiter, sigma=sigma), P2)


# ---- (g): more workgroups than the device holds at once
def test_a_grid_larger_than_the_device(sa):
    objective, n, P, maxiter, sigma, R = "sphere", 3, 6, 15, 0.3, 1100
    lower, upper = box(n)
    seeds = [3000 + r for r in range(R)]
    got = launch(objective, lower, upper, P, seeds, maxiter=maxiter, sigma=sigma)
    again = launch(objective, lower, upper, P, seeds, maxiter=maxiter, sigma=sigma)
    assert bits(got) == bits(again)
    for r in (0, 255, 256, 1023, 1024, 1099):
        pair = launch(objective, lower, upper, P, [seeds[r], seeds[r] + 5000], maxiter=maxiter, sigma=sigma)
        for k in NAMES:
            assert getattr(pair, k)[0].tobytes() == getattr(got, k)[r].tobytes(), (r, k)
    _same_run(got, 1099, oracle_run(objective, lower, upper, P, seeds[1099], maxiter=maxiter, sigma=sigma), P)
