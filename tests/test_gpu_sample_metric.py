"""GPU: per-axis scale adaptation in the warm-up (metric="diag" of stochopy_amd.sample; csrc/sx_sample.hpp metric_update, the
third form of the chain kernels in sx_sample_metric.hip and of the kernels of sx_sample_unfused.hip) against the numpy
restatement (tests/_sample_metric_oracle.py), against the adapting kernels, against itself cut into launches and around a
caller's objective, at its edges, and against the anisotropic target it is meant for.

Shapes and tolerances are tests/test_gpu_sample_adapt.py's: ndim on either side of the row-width thresholds, chains 1 / 5 /
37, 1e-6 of the span for samples, 1e-6 relative for values, multipliers and scales, counts exact.  maxiter 60 and warmup 40
give the windows (6, 16] and (16, 36]."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_metric_cases as cases  # noqa: E402
import _sample_metric_oracle  # noqa: E402
from test_gpu_sample import close_samples, close_values  # noqa: E402
from test_gpu_sample_batched import device_gradient, device_objective  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = 10.24
OUTPUTS = ("cur", "xbest", "fcur", "facc", "fmin", "iacc", "imin", "nacc", "nfeas", "xall", "funall", "scale", "hbar", "logsbar",
           "nacc_warm")
METRIC_OUTPUTS = ("sbase", "m", "mean", "M2")


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def scalars_equal(got, want, keys=("x", "fun", "nit", "accept_ratio", "accept_ratios", "accept_ratios_sampling", "stepsizes",
                                   "warmup", "nfev", "nreject", "metric", "metric_windows")):
    for key in keys:
        assert (key in got) == (key in want), key
        if key in want:
            assert np.array_equal(got[key], want[key], equal_nan=True), key


def same_arrays(got, want, names):
    for name in names:
        assert np.array_equal(got[name], want[name], equal_nan=True), name


# ---- 1: parity with the restatement -------------------------------------------------------------------------------------
def check_parity(sa, case, maxiter, warmup, windows):
    method, objective, ndim, chains, options, constraints, x0, rec = case
    bounds, start, o = cases.setup(case, maxiter, warmup)
    want = _sample_metric_oracle.sample(objective, bounds, x0=start, method=method, options=dict(o))
    got = sa.sample.sample(getattr(sa.factory, objective), bounds, x0=start, method=method, options=dict(o, backend="hip"))
    rows = len(range(rec[0] if rec else warmup, maxiter, rec[1] if rec else 1))
    assert got.xall.shape == ((chains, rows, ndim) if chains > 1 else (rows, ndim)) and got.funall.shape == got.xall.shape[:-1]
    with np.errstate(all="ignore"):
        print("max |dx| / span", np.nanmax(np.abs(got.xall - want.xall)) / SPAN, "max rel df",
              np.nanmax(np.abs(got.funall - want.funall) / np.abs(want.funall)), "max rel dstep",
              np.max(np.abs(got.stepsizes / want.stepsizes - 1.0)), "max rel dmetric", np.max(np.abs(got.metric / want.metric - 1.0)),
              "steps", np.min(want.stepsizes), "...", np.max(want.stepsizes), "metric", np.min(want.metric), "...",
              np.max(want.metric), "accept", want.accept_ratio)
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    assert got.nit == want.nit == maxiter and got.warmup == warmup and got.accept_ratio == want.accept_ratio
    if chains > 1:
        assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.array_equal(got.accept_ratios_sampling, want.accept_ratios_sampling)
    assert np.shape(got.stepsizes) == (() if chains == 1 else (chains,))
    assert np.shape(got.metric) == ((ndim,) if chains == 1 else (chains, ndim))
    assert got.metric_windows == want.metric_windows == windows
    assert np.allclose(got.stepsizes, want.stepsizes, rtol=1e-6, atol=0.0)
    assert np.allclose(got.metric, want.metric, rtol=1e-6, atol=0.0)
    assert close_samples(got.x, want.x) and close_values(got.fun, want.fun)
    if method == "hmc":
        assert got.nfev == want.nfev
    if constraints == "Reject":
        assert got.nreject == chains * (maxiter - 1) - int(want.nfeas.sum())
    assert 0 < int(want.nacc.sum()) < chains * (maxiter - 1)  # both outcomes of the decision occur
    assert not np.all(want.metric == 1.0)


@pytest.mark.parametrize("case", cases.PARITY, ids=cases.case_id)
def test_parity_with_the_restatement(sa, case):
    check_parity(sa, case, cases.MAXITER, cases.WARMUP, (16, 36))


# ---- through the C ABI --------------------------------------------------------------------------------------------------
def abi_run(method, ndim, chains, maxiter, form, warmup=15, windows=(0, ()), cuts=(), unfused=False, objective="sphere",
            fixed_axis=None, stepsize=0.02, target=None):
    """Every output array of one run of sx_sample_run_adapt (form "adapt") or sx_sample_run_metric ("metric"), launched in the
    pieces `cuts` makes of [0, maxiter) -- or, `unfused`, sample by sample around sx_eval / sx_sample_gradient through
    sx_sample_propose / _leap / _decide in the same form.  `fixed_axis`: lower == upper there."""
    import torch

    from stochopy_amd import _device, _lib

    ctx = _device.Context()
    L = ctx.L
    with torch.cuda.stream(ctx.stream):
        dev = {name: ctx.empty((chains, ndim)) for name in ("cur", "xbest")}
        dev.update({name: ctx.empty((chains,)) for name in ("fcur", "facc", "fmin")})
        dev.update({name: ctx.empty((chains,), dtype=torch.int64) for name in ("iacc", "imin", "nacc", "nfeas")})
        dev["xall"], dev["funall"] = ctx.empty((chains, maxiter, ndim)), ctx.empty((chains, maxiter))
        lower, upper = np.full(ndim, -5.12), np.full(ndim, 5.12)
        if fixed_axis is not None:
            lower[fixed_axis] = upper[fixed_axis] = 0.25
        dev["lower"], dev["upper"] = ctx.upload(lower), ctx.upload(upper)
        dev["step"] = ctx.upload(np.full(ndim, stepsize) * (0.5 * (upper - lower)))
        a = _lib.SxSampleArgs()
        for name in dev:
            setattr(a, name, _device.ptr(dev[name]))
        a.C, a.maxiter, a.x0_stride, a.n = chains, maxiter, 0, ndim
        a.fun_id = _lib.FUN_IDS[objective]
        a.method = _lib.SX_SAMPLE_MCMC if method == "mcmc" else _lib.SX_SAMPLE_HMC
        a.rng, a.reject, a.k, a.nleap, a.jac = _lib.SX_RNG_PHILOX, 1, max(1, int(0.3 * ndim)), 3, _lib.SX_JAC_ANALYTIC
        a.fd_step, a.key0, a.key1 = 1.0e-4, 17, 3
        ad = _lib.SxSampleAdapt()
        dev.update({name: ctx.empty((chains,)) for name in ("scale", "hbar", "logsbar")})
        dev["nacc_warm"] = ctx.empty((chains,), dtype=torch.int64)
        for name in ("scale", "hbar", "logsbar", "nacc_warm"):
            setattr(ad, name, _device.ptr(dev[name]))
        ad.warmup, ad.rec_start, ad.rec_every, ad.rec_rows = warmup, 0, 1, maxiter
        ad.target = target if target is not None else 0.234 if method == "mcmc" else 0.9
        mt = _lib.SxSampleMetric()
        start, ends = windows
        if ends:
            dev["sbase"] = ctx.empty((chains,))
            dev.update({name: ctx.empty((chains, ndim)) for name in ("m", "mean", "M2")})
            for name in METRIC_OUTPUTS:
                dev[name].fill_(float("nan"))  # (the launch that generates sample 0 writes them)
                setattr(mt, name, _device.ptr(dev[name]))
        mt.nwin, mt.win_start = len(ends), start
        for j, end in enumerate(ends):
            mt.win_end[j] = end
        extra = [C.byref(ad)] + ([C.byref(mt)] if form == "metric" else [])

        def call(name, *args):
            _lib.check(getattr(L, f"sx_sample_{name}_{form}")(C.byref(a), *extra, *args, ctx.stream_ptr), name)

        if not unfused:
            edges = [0] + sorted(cuts) + [maxiter]
            for lo, hi in zip(edges, edges[1:]):
                call("run", lo, hi - lo)
        else:
            prop, pmom, k0 = ctx.empty((chains, ndim)), ctx.empty((chains, ndim)), ctx.empty((chains,))
            f, G = ctx.empty((chains,)), ctx.empty((chains, ndim))
            ptr = _device.ptr

            def value():
                _lib.check(L.sx_eval(a.fun_id, ptr(prop), chains, ndim, ndim, None, None, ptr(f), None, None, ctx.stream_ptr), "sx_eval")

            for it in range(maxiter):
                call("propose", it, ptr(prop), ptr(pmom), ptr(k0))
                if method == "hmc" and it > 0:
                    for g in range(a.nleap + 2):
                        _lib.check(L.sx_sample_gradient(a.fun_id, ptr(prop), chains, ndim, ptr(G), ctx.stream_ptr), "gradient")
                        call("leap", 0.5 if g in (0, a.nleap + 1) else 1.0, int(g <= a.nleap), ptr(prop), ptr(pmom), ptr(G))
                value()
                call("decide", it, ptr(prop), ptr(f), ptr(pmom), ptr(k0))
        ctx.sync()
        return {name: dev[name].cpu().numpy() for name in OUTPUTS + (METRIC_OUTPUTS if ends else ())}


# ---- 2: nothing changes when there is no window -------------------------------------------------------------------------
@pytest.mark.parametrize("unfused", [False, True], ids=["resident", "unfused"])
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
@pytest.mark.parametrize("ndim", [3, 129])
def test_nothing_changes_when_there_is_no_window(sa, method, ndim, unfused):
    adapt = abi_run(method, ndim, 5, 25, "adapt", unfused=unfused)
    same = abi_run(method, ndim, 5, 25, "metric", unfused=unfused)  # (nwin = 0: the four metric pointers stay NULL)
    same_arrays(same, adapt, OUTPUTS)
    assert np.all(np.isfinite(adapt["funall"])) and 0 < adapt["nacc"].sum() < 5 * 24 and not np.all(adapt["scale"] == 1.0)


@pytest.mark.parametrize("method,options", [("mcmc", {"perc": 0.3}), ("hmc", {"nleap": 3, "jac": "analytic"})], ids=["mcmc", "hmc"])
def test_metric_none_is_the_call_without_the_keyword(sa, method, options):
    bounds = [[-5.12, 5.12]] * 65
    for extra in ({}, {"warmup": 25, "burn": 7, "thin": 3}):
        o = dict(options, maxiter=40, seed=8, chains=5, rng="philox", backend="hip", **extra)
        without = sa.sample.sample(sa.factory.rastrigin, bounds, method=method, options=dict(o))
        given = sa.sample.sample(sa.factory.rastrigin, bounds, method=method, options=dict(o, metric=None))
        assert np.array_equal(without.xall, given.xall) and np.array_equal(without.funall, given.funall)
        scalars_equal(given, without)
        assert "metric" not in given and "metric_windows" not in given


# ---- 3: a run does not depend on its launches or on the number of chains ------------------------------------------------
METHODS = [("mcmc", {"stepsize": 0.05, "perc": 0.3}), ("hmc", {"stepsize": 0.01, "nleap": 3, "jac": "analytic"})]


@pytest.mark.parametrize("method,options", METHODS, ids=["mcmc", "hmc"])
def test_a_run_does_not_depend_on_its_launches_or_chains(sa, method, options):
    bounds = [[-5.12, 5.12]] * 8
    o = dict(options, maxiter=60, warmup=40, metric="diag", burn=7, thin=3, seed=5, rng="philox", backend="hip")
    fun = sa.factory.rastrigin
    few = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=5))
    many = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=37))
    assert np.array_equal(few.xall, many.xall[:5]) and np.array_equal(few.funall, many.funall[:5])
    for key in ("accept_ratios", "accept_ratios_sampling", "stepsizes", "metric"):
        assert np.array_equal(few[key], many[key][:5]), key
    seen = []
    cut = sa.sample.sample(fun, bounds, method=method, options=dict(o, chains=5),
                           callback=lambda xk, state: seen.append(np.array(xk, copy=True)))  # one launch per sample
    assert len(seen) == 60 and np.array_equal(np.stack(seen, axis=1)[:, 7::3], few.xall)
    assert np.array_equal(cut.xall, few.xall) and np.array_equal(cut.funall, few.funall)
    scalars_equal(cut, few)
    assert not np.all(few.metric == 1.0) and not np.all(few.stepsizes == 1.0)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_cut_at_a_window_end_and_one_sample_before_it(sa, method):
    windows = (6, (16, 36))
    whole = abi_run(method, 65, 37, 50, "metric", warmup=40, windows=windows)
    for cuts in ((16,), (15,), (15, 16, 17, 35, 36, 40, 41)):
        same_arrays(abi_run(method, 65, 37, 50, "metric", warmup=40, windows=windows, cuts=cuts), whole, OUTPUTS + METRIC_OUTPUTS)
    assert not np.all(whole["m"] == 1.0) and np.all(whole["mean"] == 0.0) and np.all(whole["M2"] == 0.0)


# ---- 4: around a caller's objective it is the resident run --------------------------------------------------------------
@pytest.mark.parametrize("ndim", [8, 65])
@pytest.mark.parametrize("method,options,chains", [
    ("mcmc", {"stepsize": 0.05, "perc": 0.3}, 37),
    ("hmc", {"stepsize": 0.01, "nleap": 3, "jac": "analytic"}, 5),   # the caller's own (batched) gradient
    ("hmc", {"stepsize": 0.01, "nleap": 2, "jac": None}, 37),        # finite differences around the caller's objective
], ids=["mcmc", "hmc-batched-gradient", "hmc-finite-differences"])
def test_around_a_callers_objective_it_is_the_resident_run(sa, method, options, chains, ndim):
    bounds = [[-5.12, 5.12]] * ndim
    o = dict(options, maxiter=50, warmup=40, metric="diag", burn=7, thin=3, seed=12, chains=chains, constraints="Reject",
             rng="philox", backend="hip")
    fused = sa.sample.sample(sa.factory.sphere, bounds, method=method, options=dict(o))
    if o.get("jac") == "analytic":
        o["jac"] = device_gradient(sa, "sphere")
    ext = sa.sample.sample(device_objective(sa, "sphere"), bounds, method=method, options=o)
    assert np.array_equal(ext.xall, fused.xall) and np.array_equal(ext.funall, fused.funall)
    scalars_equal(ext, fused)
    assert np.all(np.isfinite(fused.funall)) and not np.all(fused.stepsizes == 1.0) and not np.all(fused.metric == 1.0)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_the_unfused_entry_points_are_the_resident_ones(sa, method):
    windows = (2, (4, 12, 20))  # (a window of two samples first)
    whole = abi_run(method, 129, 5, 30, "metric", warmup=20, windows=windows)
    same_arrays(abi_run(method, 129, 5, 30, "metric", warmup=20, windows=windows, unfused=True), whole, OUTPUTS + METRIC_OUTPUTS)
    assert not np.all(whole["m"] == 1.0)


# ---- 5: edges -----------------------------------------------------------------------------------------------------------
def restated(method, chains, maxiter, warmup, windows, seed):
    """Options of the restatement for sphere with `windows` placed freely (well conditioned: moved by one unit in the last
    place, every run below stays within 1e-10 in xall, stepsizes and metric)."""
    o = {"maxiter": maxiter, "warmup": warmup, "windows": windows, "seed": seed, "chains": chains, "burn": 0, "constraints": "Reject"}
    o.update({"perc": 0.0, "stepsize": 0.005} if method == "mcmc" else {"nleap": 3, "jac": "analytic", "stepsize": 0.02,
                                                                         "target_accept": 0.9})
    return o


EDGES = [((2, (4,)), "a window of two samples"),
         ((1, (4, 7, 10, 14, 19, 25, 32, 38)), "eight windows"),
         ((10, (25, 40)), "a window that ends at it == warmup")]


@pytest.mark.parametrize("windows,what", EDGES, ids=[e[1] for e in EDGES])
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_windows_placed_freely(sa, monkeypatch, method, windows, what):
    """The library takes the window ends as given.  Against the restatement: the public call with its schedule replaced (it
    hands the library what the schedule returns).  Then the same windows through sx_sample_run_metric, whole and cut."""
    from stochopy_amd.sample import _adapt

    o = restated(method, 5, 50, 40, windows, seed=21)
    bounds = [[-5.12, 5.12]] * 65
    want = _sample_metric_oracle.sample("sphere", bounds, method=method, options=dict(o))
    monkeypatch.setattr(_adapt, "metric_windows", lambda warmup: windows)
    public = {k: v for k, v in o.items() if k != "windows"}
    got = sa.sample.sample(sa.factory.sphere, bounds, method=method, options=dict(public, metric="diag", rng="philox", backend="hip"))
    print(what, "max rel dstep", np.max(np.abs(got.stepsizes / want.stepsizes - 1.0)), "max rel dmetric",
          np.max(np.abs(got.metric / want.metric - 1.0)), "metric", want.metric.min(), "...", want.metric.max())
    assert got.metric_windows == windows[1] == want.metric_windows
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    assert np.allclose(got.stepsizes, want.stepsizes, rtol=1e-6, atol=0.0) and np.allclose(got.metric, want.metric, rtol=1e-6, atol=0.0)
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.array_equal(got.accept_ratios_sampling, want.accept_ratios_sampling)
    assert np.max(np.abs(want.metric - 1.0)) > 1e-3 and 0 < int(want.nacc.sum()) < 5 * 49
    # the same windows through sx_sample_run_metric in one launch and in two
    whole = abi_run(method, 65, 5, 50, "metric", warmup=40, windows=windows)
    same_arrays(abi_run(method, 65, 5, 50, "metric", warmup=40, windows=windows, cuts=(windows[1][0],)), whole, OUTPUTS + METRIC_OUTPUTS)
    assert np.all(np.isfinite(whole["m"])) and np.all(whole["m"] > 0.0) and np.all(whole["mean"] == 0.0) and np.all(whole["M2"] == 0.0)
    assert np.allclose(np.exp(np.log(whole["m"]).mean(axis=1)), 1.0, rtol=1e-12)
    if windows[1][-1] == 40:  # the restart at it == warmup leaves the frozen multiplier in sbase
        assert np.array_equal(whole["sbase"], whole["scale"])


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_an_axis_of_no_width_keeps_the_scales(sa, method):
    """lower == upper on axis 1: step is 0 there, the chain never moves on it, its variance is 0 and so is the shrinkage target
    (h = 0): r = 0 is not positive and the row keeps its previous m, 1.0, at every window end -- while the step size restarts."""
    got = abi_run(method, 8, 37, 50, "metric", warmup=40, windows=(6, (16, 36)), fixed_axis=1)
    free = abi_run(method, 8, 37, 50, "metric", warmup=40, windows=(6, (16, 36)))
    assert np.all(got["m"] == 1.0) and np.all(got["mean"] == 0.0) and np.all(got["M2"] == 0.0)
    assert np.all(got["xall"][:, :, 1] == 0.25) and np.all(np.isfinite(got["funall"]))
    assert np.all(np.isfinite(got["sbase"])) and not np.all(got["sbase"] == 1.0) and 0 < got["nacc"].sum() < 37 * 49
    assert not np.all(free["m"] == 1.0)


def test_non_finite_values_keep_the_scales_and_shrink_the_step(sa):
    """tests/test_gpu_sample_adapt.py test_non_finite_values_shrink_the_step with metric="diag" (warmup 20: one window,
    (3, 18]): every chain is NaN from its second sample on, so the window's variance is NaN, the row keeps m = 1, and a NaN d
    still counts as a rejection in the dual averaging."""
    bounds = [[-1.0, 1.0]] * 4
    o = {"maxiter": 30, "warmup": 20, "metric": "diag", "stepsize": 0.05, "seed": 3, "chains": 37, "jac": "analytic", "rng": "philox"}
    want = _sample_metric_oracle.sample("rosenbrock", bounds, method="hmc", options=dict(o))
    got = sa.sample.sample(sa.factory.rosenbrock, bounds, method="hmc", options=dict(o, backend="hip"))
    print("NaN samples", int(np.isnan(want.funall_full).sum()), "of", want.funall_full.size, "steps", want.stepsizes.min(), "...",
          want.stepsizes.max(), "max rel dstep", np.max(np.abs(got.stepsizes / want.stepsizes - 1.0)))
    assert np.isnan(want.xall_full[:, 2:]).all() and np.all(want.metric == 1.0)  # (every chain, in the restatement)
    assert got.metric.shape == (37, 4) and np.all(got.metric == 1.0) and got.metric_windows == (18,)
    assert np.all(np.isfinite(got.stepsizes)) and np.all(got.stepsizes > 0.0) and np.all(got.stepsizes < 1.0)
    assert close_samples(got.xall, want.xall, span=2.0) and close_values(got.funall, want.funall)
    assert np.array_equal(np.isnan(got.xall), np.isnan(want.xall))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert np.allclose(got.stepsizes, want.stepsizes, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("case", cases.WIDE, ids=cases.case_id)
def test_the_longest_row(sa, case):
    """ndim 2048: one chain per wavefront, and with eff the analytic hmc row is 4 x 2048 doubles and its padding -- more than
    the 64 KiB a kernel gets by default."""
    check_parity(sa, case, cases.WIDE_MAXITER, cases.WIDE_WARMUP, (18,))


# ---- 6: it adapts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_it_adapts_per_axis(sa, method):
    """The anisotropic Gaussian of tests/_sample_metric_cases.py as the caller's own device objective (hmc: with the caller's
    gradient), seed 0: the statistic and the bounds of tests/test_sample_metric_host.py, which came from the restatement."""
    import torch

    sigma = torch.as_tensor(cases.SIGMA, device="cuda")
    fun = sa.factory.batched(lambda X: 0.5 * ((X / sigma) ** 2).sum(dim=1))
    slow = {}
    for metric in (None, "diag"):
        o = dict(cases.gauss_options(method, 0, metric), backend="hip")
        if method == "hmc":
            o["jac"] = sa.factory.batched(lambda X: X / sigma ** 2)
        r = sa.sample.sample(fun, cases.GAUSS_BOUNDS, x0=np.zeros(8), method=method, options=o)
        slow[metric] = cases.slowest_jump(r.xall)
    learnt = float(np.mean(r.metric[:, -1] / r.metric[:, 0]))
    print(method, "slowest axis: scalar", slow[None], "with the scales", slow["diag"], "ratio", slow["diag"] / slow[None],
          "learnt", learnt)
    assert r.metric.shape == (cases.GAUSS_CHAINS, 8)
    assert slow["diag"] / slow[None] >= cases.GAUSS_RATIO_BOUND[method]
    assert cases.SCALE_RATIO_EXACT / 2 <= learnt <= cases.SCALE_RATIO_EXACT * 2
