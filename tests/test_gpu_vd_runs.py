"""VD-CMA with options["runs"] = R on the GPU (csrc/sx_vd_runs.hip: one resident workgroup per run): run r of a batched call
is the run of its seed -- held against the numpy oracle with the tolerances the single-run device loop is held to
(tests/test_gpu_vdcma.py::test_vdcma_device_loop_matches_oracle: nit, nfev, status, success and message exactly, fun within
rtol 1e-6, x within rtol 1e-5 / atol 1e-7), one generation at a time against the oracle's probe, and against that single-run
loop itself; runs stop on their own, at different generations, and do not depend on their neighbours.

All whole-run cases: 8 runs per launch, seeds 900 ... 907, bounds [-3, 4] per variable, sigma = 0.3, rng="philox"."""
import functools
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _stop_rules  # noqa: E402
import _vd_runs_abi as abi  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = tuple(range(900, 908))
SIGMA = 0.3
LO, HI = -3.0, 4.0


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(scope="module")
def lib():
    from stochopy_amd import _lib

    return _lib.lib()


def _bounds(n):
    return [[LO, HI]] * n


def _runs(sa, obj, n, seed, x0=None, bounds=None, **opts):
    return sa.optimize.minimize(getattr(sa.factory, obj), _bounds(n) if bounds is None else bounds, x0=x0, method="vdcma",
                                options=dict(dict(sigma=SIGMA), **opts, seed=seed, backend="hip", rng="philox"))


@functools.lru_cache(maxsize=None)
def _oracle(obj, n, P, maxiter, seed, extra=()):
    """One oracle run; computed once, shared by the tests that need it (treated as read-only)."""
    return oracle.minimize(obj, _bounds(n), method="vdcma", rng="philox",
                           options=dict(dict(extra), maxiter=maxiter, popsize=P, seed=seed, sigma=SIGMA))


def _same_run(got, r, ref, P, counts=True):
    """Run r of a batched result against a single run's result, with the single-run loop's tolerances."""
    status = int(got.statuses[r])
    if counts:
        assert (int(got.nits[r]), int(got.nits[r]) * P) == (ref.nit, ref.nfev), (r, int(got.nits[r]), ref.nit)
    assert (status, status >= 0) == (ref.status, ref.success), (r, status, ref.status)
    assert np.isclose(got.funs[r], ref.fun, rtol=1e-6, atol=1e-300), (r, got.funs[r], ref.fun)
    assert np.allclose(got.xs[r], ref.x, rtol=1e-5, atol=1e-7), (r, got.xs[r], ref.x)


# (objective, n, popsize, maxiter, extra options, the status the oracle ends with, its nit range).  For every case and seed
# the oracle alone, with sigma nudged by one ulp either way, keeps nit and status and moves fun by at most 7e-8 (relative).
# n: the smallest the kernel takes (6), 7 with the smallest population, the 16-lane rows' one and two Philox calls per lane
# (16 | 17, 32 | 33), the last 16-lane row (64) and the first 32-lane row (65), the last 32-lane row (128), whole-wave rows
# (130), the row stride's change at 256 | 257, a row beyond 512; popsize 70: the ranking's second 64-key chunk.
TABLE = [("sphere", 6, 6, 300, (), 1, (80, 112)),
         ("sphere", 7, 4, 600, (), 1, (138, 196)),
         ("rosenbrock", 6, 8, 400, (), -1, (400, 400)),
         ("sphere", 16, 10, 400, (), 1, (134, 155)),
         ("rosenbrock", 17, 12, 150, (), -1, (150, 150)),
         ("quartic", 20, 9, 100, (), -1, (100, 100)),
         ("sphere", 12, 70, 60, (), -1, (60, 60)),
         ("rastrigin", 33, 14, 120, (), -1, (120, 120)),
         ("sphere", 40, 10, 600, (("ftol", 1e-9),), 1, (308, 354)),
         ("ackley", 64, 16, 120, (), -1, (120, 120)),
         ("sphere", 65, 16, 200, (), -1, (200, 200)),
         ("griewank", 128, 18, 80, (), -1, (80, 80)),
         ("rosenbrock", 130, 24, 60, (), -1, (60, 60)),
         ("styblinski_tang", 257, 20, 40, (), -1, (40, 40)),
         ("sphere", 600, 32, 30, (), -1, (30, 30)),
         ("sphere", 6, 6, 3000, (("ftol", -1.0),), -5, (138, 179)),
         # (the feature request announced "-5 x 7, -1 x 1" for the next shape; the oracle ends all eight seeds by rule -5)
         ("sphere", 33, 12, 400, (("ftol", -1.0),), -5, (336, 371)),
         # rule 0 needs |xmean - xold| <= xtol in the first generation with fbest < ftol: with xtol = 1e-2 every run of the two
         # sphere cases above ends by it, at the generation where rule 1 would have ended it
         ("sphere", 6, 6, 300, (("xtol", 1e-2),), 0, (80, 112)),
         ("sphere", 16, 10, 400, (("xtol", 1e-2),), 0, (134, 155))]
_ID = lambda c: "%s_n%d_p%d_it%d" % c[:4] + ("_%s%g" % c[4][0] if len(c) > 4 and c[4] else "")  # noqa: E731


@pytest.mark.parametrize("cfg", TABLE, ids=_ID)
def test_every_run_against_the_oracle(sa, cfg):
    obj, n, P, maxiter, extra, status, (lo, hi) = cfg
    got = _runs(sa, obj, n, list(SEEDS), runs=len(SEEDS), maxiter=maxiter, popsize=P, **dict(extra))
    refs = [_oracle(obj, n, P, maxiter, s, extra) for s in SEEDS]
    print(cfg[:5], "nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    print("  oracle nit", [ref.nit for ref in refs], "status", [ref.status for ref in refs])
    print("  rel fun", ["%.3g" % (abs(got.funs[r] - ref.fun) / max(abs(ref.fun), 1e-300)) for r, ref in enumerate(refs)])
    for ref in refs:  # (what the case is there for)
        assert lo <= ref.nit <= hi and ref.status == status
    for r, ref in enumerate(refs):
        _same_run(got, r, ref, P)
        assert sa.optimize._common.messages[int(got.statuses[r])] == ref.message
    if status == 1:  # the runs end at different generations: workgroups exit at different times
        assert len(set(int(v) for v in got.nits)) > 3


def test_rule_minus_3_against_the_oracle(sa):
    """Rule -3 (TolXUp's neighbour `any(0.2 sigma sqrt(diagC) < 1e-10)`) is reached by (rastrigin, 8, 8, maxiter 3000), nit
    196 ... 259.  There the ORACLE ALONE changes nit when sigma is nudged by one ulp (fun does not move), so nit and nfev are
    not compared: status, fun and x only."""
    obj, n, P, maxiter = "rastrigin", 8, 8, 3000
    got = _runs(sa, obj, n, list(SEEDS), runs=len(SEEDS), maxiter=maxiter, popsize=P)
    refs = [_oracle(obj, n, P, maxiter, s) for s in SEEDS]
    print("rule -3: nit", [int(v) for v in got.nits], "oracle nit", [ref.nit for ref in refs], "status", [int(v) for v in got.statuses])
    for r, ref in enumerate(refs):
        assert ref.status == -3 and 196 <= ref.nit <= 259
        _same_run(got, r, ref, P, counts=False)


@pytest.mark.parametrize("rule", [-3, -6, -7, -8])
def test_the_other_stop_rules_against_the_oracle(sa, rule):
    """The rules TABLE does not reach (it has -1, 0, 1 and -5; -3 above without its counts), by the recipes of
    tests/_stop_rules.py at n = 8, popsize 10: the seeds the oracle alone admits, in one launch, each held to its oracle run --
    nit, nfev and status exactly, fun and x with this module's tolerances."""
    n = 8
    keep, table = _stop_rules.vd_admitted(rule, n)
    obj, bounds, x0, opts = _stop_rules.vd_case(rule, n)
    print("rule", rule, obj, opts)
    print("\n".join(table))
    got = _runs(sa, obj, n, [s for s, _ in keep], x0=x0, bounds=bounds, runs=len(keep), **opts)
    print("  device nit", [int(v) for v in got.nits], "status", [int(v) for v in got.statuses])
    print("  rel fun", ["%.3g" % (abs(got.funs[r] - ref.fun) / max(abs(ref.fun), 1e-300)) for r, (_, ref) in enumerate(keep)])
    for r, (_, ref) in enumerate(keep):
        _same_run(got, r, ref, opts["popsize"])


@functools.lru_cache(maxsize=None)
def _probed(obj, n, P, gens, seed):
    steps = []
    oracle.minimize(obj, _bounds(n), method="vdcma", rng="philox",
                    options=dict(maxiter=gens, popsize=P, sigma=SIGMA, seed=seed,
                                 probe=lambda it, before, after: steps.append(after)))
    assert len(steps) == gens
    return steps


def _close(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("cfg", [("rosenbrock", 12, 16), ("rastrigin", 130, 24), ("sphere", 257, 10)], ids=lambda c: "%s_n%d_p%d" % c)
def test_one_generation_at_a_time_against_the_oracle_probe(sa, cfg):
    """maxiter = 1 ... 6 through the C ABI with the optional outputs: the model a run of g generations ends with is the
    oracle's after its generation g -- mean (1e-11), sigma (1e-10), d and v (1e-9), the best row and its value: the tolerances of
    tests/test_gpu_vdcma.py::test_device_loop_generation_by_generation_from_the_oracles_state.  A wrong injection row, rank gap
    or moment shows here first (generation 2 is the first with the injection, generation 3 the first that samples from a
    model the injection has moved)."""
    obj, n, P = cfg
    gens = 6
    xm, xstd = 0.5 * (HI + LO), 0.5 * (HI - LO)
    for g in range(1, gens + 1):
        out = abi.launch_runs(obj, [LO] * n, [HI] * n, P, SEEDS, maxiter=g, sigma=SIGMA)
        assert (out["nits"] == g).all() and (out["statuses"] == -1).all()
        for r, s in enumerate(SEEDS):
            after = _probed(obj, n, P, gens, s)[g - 1]
            best = int(after["order"][0])
            assert _close(out["xmeans"][r], after["xmean"], 1e-11), (g, r)
            assert np.isclose(out["sigmas"][r], after["sigma"], rtol=1e-10, atol=0), (g, r, out["sigmas"][r], after["sigma"])
            assert _close(out["dvecs"][r], after["dvec"], 1e-9), (g, r)
            assert _close(out["vvecs"][r], after["vvec"], 1e-9), (g, r)
            assert _close(out["xs"][r], after["arx"][best] * xstd + xm, 1e-11), (g, r)
            assert np.isclose(out["funs"][r], after["arfit"][best], rtol=1e-9, atol=1e-300), (g, r)


def _bits(res):
    return res.xs.tobytes(), res.funs.tobytes(), res.nits.tobytes(), res.statuses.tobytes(), res.sigmas.tobytes()


INDEP = ("rosenbrock", 17, 12, 60)


def test_a_run_does_not_depend_on_its_neighbours(sa):
    obj, n, P, maxiter = INDEP
    R = len(SEEDS)
    opts = dict(maxiter=maxiter, popsize=P)
    whole = _runs(sa, obj, n, list(SEEDS), runs=R, **opts)
    again = _runs(sa, obj, n, list(SEEDS), runs=R, **opts)
    assert _bits(whole) == _bits(again)  # nothing stale is read: LDS, workspace
    by_offset = _runs(sa, obj, n, SEEDS[0], runs=R, **opts)  # seed + r
    assert _bits(whole) == _bits(by_offset)
    for r in range(R):
        pair = _runs(sa, obj, n, [SEEDS[r], SEEDS[r] + 100], runs=2, **opts)
        assert (pair.xs[0] == whole.xs[r]).all() and pair.funs[0] == whole.funs[r] and pair.sigmas[0] == whole.sigmas[r]
        assert pair.nits[0] == whole.nits[r] and pair.statuses[0] == whole.statuses[r]
    back = _runs(sa, obj, n, list(reversed(SEEDS)), runs=R, **opts)
    assert (back.xs[::-1] == whole.xs).all() and (back.funs[::-1] == whole.funs).all()
    assert (back.nits[::-1] == whole.nits).all() and (back.statuses[::-1] == whole.statuses).all()


def test_a_grid_larger_than_the_device(sa):
    """R = 1100 workgroups (more than are resident at once): the first 8 are the 8 of the small launch, bit for bit."""
    obj, n, P, maxiter = "sphere", 16, 10, 400
    few = _runs(sa, obj, n, SEEDS[0], runs=len(SEEDS), maxiter=maxiter, popsize=P)
    many = _runs(sa, obj, n, SEEDS[0], runs=1100, maxiter=maxiter, popsize=P)
    k = len(SEEDS)
    assert (many.xs[:k] == few.xs).all() and (many.funs[:k] == few.funs).all() and (many.sigmas[:k] == few.sigmas).all()
    assert (many.nits[:k] == few.nits).all() and (many.statuses[:k] == few.statuses).all()
    assert (many.statuses == 1).all() and (many.nits > 100).all() and (many.nits < 250).all() and (many.funs <= 1e-8).all()
    assert many.nfev == int(many.nits.sum()) * P


def test_x0_per_run_or_shared(sa):
    obj, n, P, maxiter = "rosenbrock", 17, 12, 40
    R = len(SEEDS)
    X = np.random.RandomState(3).uniform(-2.0, 3.0, (R, n))
    kept = X.copy()
    opts = dict(maxiter=maxiter, popsize=P)
    per_run = _runs(sa, obj, n, list(SEEDS), x0=X, runs=R, **opts)
    assert (X == kept).all()
    for r in range(R):
        shared = _runs(sa, obj, n, [SEEDS[r], SEEDS[r] + 1000], x0=X[r], runs=2, **opts)
        assert (shared.xs[0] == per_run.xs[r]).all() and shared.funs[0] == per_run.funs[r]
        assert shared.nits[0] == per_run.nits[r] and shared.statuses[0] == per_run.statuses[r]
    # and x0 is the caller's point (the direction is then the FIRST draw of the run's stream): the single run from it
    ref = _runs(sa, obj, n, SEEDS[2], x0=X[2], **opts)
    _same_run(per_run, 2, ref, P)


@pytest.mark.parametrize("cfg", [("rosenbrock", 17, 12, 60), ("sphere", 65, 16, 60), ("rastrigin", 130, 24, 40),
                                 ("styblinski_tang", 257, 20, 30)], ids=_ID)
def test_every_run_against_the_single_run_device_loop(sa, cfg):
    obj, n, P, maxiter = cfg
    got = _runs(sa, obj, n, list(SEEDS), runs=len(SEEDS), maxiter=maxiter, popsize=P)
    for r, s in enumerate(SEEDS):
        ref = _runs(sa, obj, n, s, maxiter=maxiter, popsize=P)
        _same_run(got, r, ref, P)


def _limit_shapes(lib):
    """(n, P, maxiter): the largest population of n = 6 and of n = 512, and each side of 64 KiB of LDS (where the launch
    raises the kernel's dynamic-LDS attribute) at n = 64."""
    k = abi.largest_popsize_below(64 * 1024, 64)
    return [(6, abi.largest_popsize(lib, 6), 3), (512, abi.largest_popsize(lib, 512), 3), (64, k, 5), (64, k + 1, 5)]


@pytest.mark.parametrize("which", range(4), ids=["n6_pmax", "n512_pmax", "n64_below_64KiB", "n64_above_64KiB"])
def test_whole_runs_at_the_lds_limits(sa, lib, which):
    n, P, maxiter = _limit_shapes(lib)[which]
    bytes_ = lib.sx_vd_runs_lds_bytes(P, n)
    print("n", n, "P", P, "LDS bytes", bytes_)
    assert 0 < bytes_ <= abi.LDS_LIMIT
    if which < 2:
        assert lib.sx_vd_runs_lds_bytes(P + 1, n) < 0
    else:
        assert (bytes_ <= 64 * 1024) == (which == 2) and abs(bytes_ - 64 * 1024) <= 32
    seeds = SEEDS[:4]
    got = _runs(sa, "sphere", n, list(seeds), runs=len(seeds), maxiter=maxiter, popsize=P)
    for r, s in enumerate(seeds):
        _same_run(got, r, _oracle("sphere", n, P, maxiter, s), P)


def test_a_box_per_dimension(sa):
    """No centre is 0, no two half-widths are equal: an element centred or scaled with another element's constants shows."""
    obj, n, P, maxiter = "rosenbrock", 20, 12, 60
    i = np.arange(n, dtype=np.float64)
    bounds = np.stack([-1.0 - i / 7.0, 2.0 + i / 3.0], axis=1)
    got = _runs(sa, obj, n, list(SEEDS), bounds=bounds, runs=len(SEEDS), maxiter=maxiter, popsize=P)
    for r, s in enumerate(SEEDS):
        ref = oracle.minimize(obj, bounds, method="vdcma", rng="philox", options=dict(maxiter=maxiter, popsize=P, seed=s, sigma=SIGMA))
        _same_run(got, r, ref, P)


@pytest.mark.parametrize("n,P", [(7, 12), (12, 70), (130, 9)])
def test_ranking_when_every_row_ties_at_inf(sa, n, P):
    """sphere on [-5e154, 5e154]^n from points at 0.6 ... 0.95 of the half-width: every candidate's value is +inf, np.argsort's
    stable order is the index order, so the new mean is the weighted sum of rows 0 ... mu - 1 and the best row is row 0 -- held
    to a plain numpy generation 1 (tests/_vd_runs_abi.py generation_one).  The candidates differ by sigma |y| ~ 1e-3 of the
    half-width, so a ranking that breaks ties any other way moves the mean by ~1e-4; the bound is the rounding of a sum of
    mu <= 35 products of magnitude <= 1, (mu + 2) 2^-53 < 5e-15, plus the device's few-ulp normals scaled by sigma = 2^-10."""
    half = 5e154
    sigma = 2.0 ** -10
    R = len(SEEDS)
    r_, i_ = np.arange(R)[:, None], np.arange(n)[None, :]
    x0 = half * (0.6 + 0.35 * ((7 * r_ + 3 * i_) % 11) / 11.0)
    out = abi.launch_runs("sphere", [-half] * n, [half] * n, P, SEEDS, x0=x0, maxiter=1, sigma=sigma)
    assert np.isposinf(out["funs"]).all() and (out["statuses"] == -1).all() and (out["nits"] == 1).all()
    for r, s in enumerate(SEEDS):
        ref = abi.generation_one(lambda X: (X * X).sum(axis=1), [-half] * n, [half] * n, P, s, x0[r], sigma)
        assert np.isposinf(ref["fit"]).all() and (ref["order"] == np.arange(P)).all()
        assert np.abs(out["xmeans"][r] - ref["xmean"]).max() <= 1e-14, (r, np.abs(out["xmeans"][r] - ref["xmean"]).max())
        assert np.allclose(out["xs"][r], ref["x"], rtol=1e-14, atol=0), r


def test_the_result_describes_the_best_run(sa):
    obj, n, P, maxiter = "sphere", 7, 4, 600
    R = len(SEEDS)
    res = _runs(sa, obj, n, SEEDS[0], runs=R, maxiter=maxiter, popsize=P)
    best = int(np.argmin(res.funs))
    assert res.run == best and (res.x == res.xs[best]).all() and res.fun == res.funs[best]
    assert res.nit == res.nits[best] and res.status == res.statuses[best] and res.success == (res.status >= 0)
    assert res.message == sa.optimize._common.messages[res.status]
    assert res.nfev == int(res.nits.sum()) * P
    assert res.xs.shape == (R, n) and res.xs.dtype == np.float64 and res.x.shape == (n,)
    assert res.funs.shape == res.sigmas.shape == (R,) and res.funs.dtype == res.sigmas.dtype == np.float64
    assert res.nits.shape == (R,) and res.nits.dtype == np.int64
    assert res.statuses.shape == (R,) and res.statuses.dtype == np.int32
    assert (res.sigmas > 0.0).all() and np.isfinite(res.sigmas).all()
    # the step sizes are the oracle's final ones
    for r, s in enumerate(SEEDS):
        steps = []
        oracle.minimize(obj, _bounds(n), method="vdcma", rng="philox",
                        options=dict(maxiter=maxiter, popsize=P, sigma=SIGMA, seed=s, probe=lambda it, b, a: steps.append(a["sigma"])))
        assert len(steps) == res.nits[r] and np.isclose(res.sigmas[r], steps[-1], rtol=1e-6, atol=0), r
