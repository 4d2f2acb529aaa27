"""GPU: per-chain step-size adaptation in a warm-up, burn-in and thinning (options warmup / target_accept / burn / thin of
stochopy_amd.sample; csrc/sx_sample.hpp adapt_update, the adapting kernels of sx_sample.hip and sx_sample_unfused.hip)
against the numpy restatement (tests/_sample_adapt_oracle.py), against the plain kernels, against itself cut into launches
and around a caller's objective, and against the distribution it is meant to sample.

Shapes: one case per row width (ndim 3, 64 | 65, 128 | 129, 300: 16, 32 and 64 lanes per chain on either side of each
threshold), chains 1 / 5 / 37 (a last workgroup that is partly inactive), block lengths that do not divide ndim.
Tolerances are test_gpu_sample.py's (1e-6 of the span for samples, 1e-6 relative for values, counts exact); the multipliers
agree to rtol 1e-6: with equal decisions the two sides differ by rounding only (exp, no contraction on either side), and an
error of 1e-13 in alpha reaches logs multiplied by at most sqrt(40) / 0.05 ~ 127."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_adapt_cases as cases  # noqa: E402
import _sample_adapt_oracle  # noqa: E402
from test_gpu_sample import close_samples, close_values  # noqa: E402
from test_gpu_sample_batched import device_gradient, device_objective  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = 10.24
OUTPUTS = ("cur", "xbest", "fcur", "facc", "fmin", "iacc", "imin", "nacc", "nfeas", "xall", "funall")


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def scalars_equal(got, want, keys=("x", "fun", "nit", "accept_ratio", "accept_ratios", "accept_ratios_sampling", "stepsizes",
                                   "warmup", "nfev", "nreject")):
    for key in keys:
        assert (key in got) == (key in want), key
        if key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), key


# ---- 1: parity with the restatement -------------------------------------------------------------------------------------
# The cases and why hmc sets target_accept: tests/_sample_adapt_cases.py (the rule is a feedback loop, and where it is
# ill-conditioned -- the restatement itself moves by a third of the range under a change in the last place -- a parity
# tolerance tests the rounding, not the kernel; every case here moves by less than 1e-9 of the range under that experiment).
@pytest.mark.parametrize("case", cases.PARITY, ids=cases.case_id)
def test_parity_with_the_restatement(sa, case):
    method, objective, ndim, chains, options, constraints, x0, rec = case
    bounds, start, o = cases.setup(case)
    want = _sample_adapt_oracle.sample(objective, bounds, x0=start, method=method, options=dict(o))
    got = sa.sample.sample(getattr(sa.factory, objective), bounds, x0=start, method=method, options=dict(o, backend="hip"))
    rows = len(range(rec[0] if rec else 40, 60, rec[1] if rec else 1))
    assert got.xall.shape == ((chains, rows, ndim) if chains > 1 else (rows, ndim)) and got.funall.shape == got.xall.shape[:-1]
    with np.errstate(all="ignore"):
        print("max |dx| / span", np.nanmax(np.abs(got.xall - want.xall)) / SPAN, "max rel df",
              np.nanmax(np.abs(got.funall - want.funall) / np.abs(want.funall)), "max rel dstep",
              np.max(np.abs(got.stepsizes / want.stepsizes - 1.0)), "steps", np.min(want.stepsizes), "...",
              np.max(want.stepsizes), "accept", want.accept_ratio, "infeasible", chains * 59 - int(want.nfeas.sum()))
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    assert got.nit == want.nit == 60 and got.warmup == 40 and got.accept_ratio == want.accept_ratio
    if chains > 1:
        assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.array_equal(got.accept_ratios_sampling, want.accept_ratios_sampling)
    assert np.shape(got.stepsizes) == (() if chains == 1 else (chains,))
    assert np.allclose(got.stepsizes, want.stepsizes, rtol=1e-6, atol=0.0)
    assert close_samples(got.x, want.x) and close_values(got.fun, want.fun)
    if method == "hmc":
        assert got.nfev == want.nfev
    if constraints == "Reject":
        assert got.nreject == chains * 59 - int(want.nfeas.sum())
    assert 0 < int(want.nacc.sum()) < chains * 59  # both outcomes of the decision occur


# ---- 2: nothing changes when nothing adapts (through the C ABI) ---------------------------------------------------------
def abi_run(method, ndim, chains, maxiter, adapt):
    """Every output array of one whole run of sx_sample_run (adapt None) or sx_sample_run_adapt."""
    import torch

    from stochopy_amd import _device, _lib

    ctx = _device.Context()
    with torch.cuda.stream(ctx.stream):
        dev = {name: ctx.empty((chains, ndim)) for name in ("cur", "xbest")}
        dev.update({name: ctx.empty((chains,)) for name in ("fcur", "facc", "fmin")})
        dev.update({name: ctx.empty((chains,), dtype=torch.int64) for name in ("iacc", "imin", "nacc", "nfeas")})
        dev["xall"], dev["funall"] = ctx.empty((chains, maxiter, ndim)), ctx.empty((chains, maxiter))
        lower, upper = np.full(ndim, -5.12), np.full(ndim, 5.12)
        dev["lower"], dev["upper"] = ctx.upload(lower), ctx.upload(upper)
        dev["step"] = ctx.upload(np.full(ndim, 0.02) * (0.5 * (upper - lower)))
        a = _lib.SxSampleArgs()
        for name in dev:
            setattr(a, name, _device.ptr(dev[name]))
        a.C, a.maxiter, a.x0_stride, a.n = chains, maxiter, 0, ndim
        a.fun_id = _lib.FUN_IDS["sphere"]
        a.method = _lib.SX_SAMPLE_MCMC if method == "mcmc" else _lib.SX_SAMPLE_HMC
        a.rng, a.reject, a.k, a.nleap, a.jac = _lib.SX_RNG_PHILOX, 1, max(1, int(0.3 * ndim)), 3, _lib.SX_JAC_ANALYTIC
        a.fd_step, a.key0, a.key1 = 1.0e-4, 17, 3
        if adapt is None:
            _lib.check(ctx.L.sx_sample_run(C.byref(a), 0, maxiter, ctx.stream_ptr), "sx_sample_run")
        else:
            ad = _lib.SxSampleAdapt()  # (the four state pointers stay NULL: warmup == 0)
            ad.warmup, ad.rec_start, ad.rec_every, ad.rec_rows, ad.target = 0, 0, 1, maxiter, 0.0
            _lib.check(ctx.L.sx_sample_run_adapt(C.byref(a), C.byref(ad), 0, maxiter, ctx.stream_ptr), "sx_sample_run_adapt")
        ctx.sync()
        return {name: dev[name].cpu().numpy() for name in OUTPUTS}


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
@pytest.mark.parametrize("ndim", [3, 65, 129])
def test_nothing_changes_when_nothing_adapts(sa, method, ndim):
    plain = abi_run(method, ndim, 5, 25, None)
    same = abi_run(method, ndim, 5, 25, "off")
    for name in OUTPUTS:
        assert np.array_equal(plain[name], same[name]), name
    assert np.all(np.isfinite(plain["funall"])) and 0 < plain["nacc"].sum() < 5 * 24


# ---- 3: thinning is only recording --------------------------------------------------------------------------------------
METHODS = [("mcmc", {"stepsize": 0.05, "perc": 0.3}), ("hmc", {"stepsize": 0.01, "nleap": 3, "jac": "analytic"})]


@pytest.mark.parametrize("method,options", METHODS, ids=["mcmc", "hmc"])
def test_thinning_is_only_recording(sa, method, options):
    bounds = [[-5.12, 5.12]] * 65
    o = dict(options, maxiter=40, warmup=20, seed=8, chains=5, rng="philox", backend="hip")
    whole = sa.sample.sample(sa.factory.rastrigin, bounds, method=method, options=dict(o, burn=0, thin=1))
    thinned = sa.sample.sample(sa.factory.rastrigin, bounds, method=method, options=dict(o, burn=7, thin=3))
    assert whole.xall.shape == (5, 40, 65) and thinned.xall.shape == (5, 11, 65)
    assert np.array_equal(thinned.xall, whole.xall[:, 7::3]) and np.array_equal(thinned.funall, whole.funall[:, 7::3])
    scalars_equal(thinned, whole)
    last = sa.sample.sample(sa.factory.rastrigin, bounds, method=method, options=dict(o, burn=39, thin=1000))
    assert np.array_equal(last.xall, whole.xall[:, 39:]) and np.array_equal(last.funall, whole.funall[:, 39:])


# ---- 4: a run does not depend on its launches ---------------------------------------------------------------------------
@pytest.mark.parametrize("method,options", METHODS, ids=["mcmc", "hmc"])
def test_a_run_does_not_depend_on_its_launches(sa, method, options):
    bounds = [[-5.12, 5.12]] * 8
    o = dict(options, maxiter=40, warmup=25, burn=7, thin=3, seed=5, rng="philox", backend="hip")
    fun = sa.factory.rastrigin
    few = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=6))
    many = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=37))
    assert np.array_equal(few.xall[5], many.xall[5]) and np.array_equal(few.funall[5], many.funall[5])
    for key in ("accept_ratios", "accept_ratios_sampling", "stepsizes"):
        assert few[key][5] == many[key][5], key
    seen, states = [], []

    def callback(xk, state):
        seen.append(np.array(xk, copy=True))
        states.append(state.xall.shape[1])

    cut = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=6), callback=callback)
    assert len(seen) == 40  # one call per GENERATED sample, with that sample
    assert np.array_equal(np.stack(seen, axis=1)[:, 7::3], few.xall)
    assert np.array_equal(cut.xall, few.xall) and np.array_equal(cut.funall, few.funall)
    scalars_equal(cut, few)
    # the state's xall: the recorded rows among the samples before the newest (the first sample while there is none)
    assert states == [len([r for r in range(7, 40, 3) if r < max(i, 1)]) for i in range(40)]
    assert not np.all(few.stepsizes == 1.0)


# ---- 5: fused equals unfused --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,options,ndim,chains", [
    ("mcmc", {"stepsize": 0.05, "perc": 0.3}, 65, 37),
    ("hmc", {"stepsize": 0.01, "nleap": 3, "jac": "analytic"}, 129, 5),   # the caller's own (batched) gradient
    ("hmc", {"stepsize": 0.01, "nleap": 2, "jac": None}, 8, 37),          # finite differences around the caller's objective
], ids=["mcmc", "hmc-batched-gradient", "hmc-finite-differences"])
def test_around_a_callers_objective_it_is_the_resident_run(sa, method, options, ndim, chains):
    bounds = [[-5.12, 5.12]] * ndim
    o = dict(options, maxiter=30, warmup=20, burn=7, thin=3, seed=12, chains=chains, constraints="Reject", rng="philox",
             backend="hip")
    fused = sa.sample.sample(sa.factory.sphere, bounds, method=method, options=dict(o))
    if o.get("jac") == "analytic":
        o["jac"] = device_gradient(sa, "sphere")
    ext = sa.sample.sample(device_objective(sa, "sphere"), bounds, method=method, options=o)
    assert np.array_equal(ext.xall, fused.xall) and np.array_equal(ext.funall, fused.funall)
    scalars_equal(ext, fused)
    assert np.all(np.isfinite(fused.funall)) and not np.all(fused.stepsizes == 1.0)


# ---- 6: it adapts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,steps,accept_band", [("mcmc", (0.5, 0.001), (0.15, 0.30)), ("hmc", (0.2, 0.0005), (0.6, 0.95))])
def test_it_adapts(sa, method, steps, accept_band):
    """sphere, ndim 8, bounds +-5, 256 chains, seed 0, 800 samples of which 300 adapt; exp(-sum x^2) has variance 0.5.  The
    bands are conditions on inputs for which the restatement sits well inside (test_sample_adapt_host.py re-checks:
    acceptance 0.194 / 0.205 and 0.756 / 0.807, variance 0.503 / 0.502 and 0.504 / 0.498, ratio of steps 1.024 / 1.013;
    without a warm-up the variance is 0.998 / 8.09 for mcmc and 3.99 for hmc from 0.0005)."""
    effective = []
    for s in steps:
        o = {"maxiter": 800, "warmup": 300, "seed": 0, "chains": 256, "stepsize": s, "rng": "philox", "backend": "hip"}
        if method == "hmc":
            o["jac"] = "analytic"
        r = sa.sample.sample(sa.factory.sphere, [[-5.0, 5.0]] * 8, method=method, options=o)
        accept, var = float(r.accept_ratios_sampling.mean()), float(r.xall.var())
        effective.append(float((r.stepsizes * s).mean()))
        print(method, "stepsize", s, "acceptance", accept, "pooled variance", var, "effective step", effective[-1])
        assert r.xall.shape == (256, 500, 8) and r.warmup == 300
        assert accept_band[0] <= accept <= accept_band[1]
        assert 0.45 <= var <= 0.55
    print(method, "ratio of the mean effective steps", effective[0] / effective[1])
    assert 0.9 <= effective[0] / effective[1] <= 1.1


# ---- 7: non-finite values -----------------------------------------------------------------------------------------------
def test_non_finite_values_shrink_the_step(sa):
    """hmc on rosenbrock, bounds +-1, with a step near the leap-frog's stability limit: the first sample is finite, the
    multiplier jumps to about 10, and the second trajectory of every chain overflows to NaN.  A NaN d accepts (the project's
    rule, so the chain stays NaN) but counts as a rejection in the adaptation: the step shrinks instead of growing."""
    bounds = [[-1.0, 1.0]] * 4
    o = {"maxiter": 30, "warmup": 20, "stepsize": 0.05, "seed": 3, "chains": 37, "jac": "analytic", "rng": "philox"}
    want = _sample_adapt_oracle.sample("rosenbrock", bounds, method="hmc", options=dict(o))
    got = sa.sample.sample(sa.factory.rosenbrock, bounds, method="hmc", options=dict(o, backend="hip"))
    print("NaN samples", int(np.isnan(want.funall_full).sum()), "of", want.funall_full.size, "steps", want.stepsizes.min(), "...",
          want.stepsizes.max(), "max rel dstep", np.max(np.abs(got.stepsizes / want.stepsizes - 1.0)))
    assert np.all(np.isfinite(got.stepsizes)) and np.all(got.stepsizes > 0.0)
    assert np.isnan(want.funall_full[:, 2:]).all() and np.isfinite(want.funall_full[:, 0]).all()
    assert np.isfinite(want.funall_full[:, 1]).sum() >= 30  # (the first trajectory is finite in nearly every chain)
    assert close_samples(got.xall, want.xall, span=2.0) and close_values(got.funall, want.funall)
    assert np.array_equal(np.isnan(got.xall), np.isnan(want.xall))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.array_equal(got.accept_ratios_sampling, want.accept_ratios_sampling)
    assert np.allclose(got.stepsizes, want.stepsizes, rtol=1e-6, atol=0.0)
    assert got.nfev == want.nfev and got.accept_ratio == want.accept_ratio
