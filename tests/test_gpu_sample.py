"""GPU: stochopy_amd.sample (csrc/sx_sample.hip: one device-resident chain per row group) against the reference's recorded
runs (numpy-legacy draws, tests/golden/sample.*), against the numpy restatement (Philox draws, tests/_sample_oracle.py),
and against the distribution it is meant to sample.  Tolerances are the project's parity tolerances (conftest
check_long_case): 1e-6 of the search range for samples, 1e-6 relative for objective values; counts are exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_oracle  # noqa: E402
from conftest import GOLDEN, load_golden, unhex  # noqa: E402
from test_sample_host import case_setup, check_callback_records, recorder  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = load_golden("sample.json")["cases"]
SPAN = 10.24
ALL = ["ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang"]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def close_samples(got, want, span=SPAN):
    return np.allclose(got, want, rtol=0, atol=1e-6 * span, equal_nan=True)


def close_values(got, want):
    return np.allclose(got, want, rtol=1e-6, atol=0, equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_parity_with_the_reference(sa, case):
    """Every recorded run of the reference through stochopy_amd.sample with the reference's own stream."""
    arrays = np.load(os.path.join(GOLDEN, "sample_xall.npz"))
    bounds, x0 = case_setup(case)
    records = []
    saved = np.random.get_state()
    try:
        res = sa.sample.sample(getattr(sa.factory, case["objective"]), bounds, x0=x0, method=case["method"],
                               options=dict(case["options"], backend="hip", rng="numpy-legacy"),
                               callback=recorder(records) if "callback" in case else None)
        after = np.random.rand(4)
    finally:
        np.random.set_state(saved)
    ref = case["result"]
    want_x, want_f = arrays[case["tag"] + "__xall"], arrays[case["tag"] + "__funall"]
    with np.errstate(all="ignore"):
        print(case["tag"], "max |dx| / range", np.abs(res.xall - want_x).max() / SPAN, "max rel df",
              np.max(np.abs(res.funall - want_f) / np.abs(want_f)), "accept_ratio", res.accept_ratio)
    assert res.xall.shape == want_x.shape and res.funall.shape == want_f.shape
    assert close_samples(res.xall, want_x)
    assert close_values(res.funall, want_f)
    assert res.nit == ref["nit"] and res.accept_ratio == unhex(ref["accept_ratio"])  # (the accept count over maxiter)
    assert close_samples(res.x, unhex(ref["x"])) and close_values(res.fun, unhex(ref["fun"]))
    if case["method"] == "hmc":
        assert res.nfev == ref["nfev"]
    assert np.array_equal(after, unhex(case["next_draws"]))  # numpy's global stream is where the reference leaves it
    if "callback" in case:
        check_callback_records(records, case["callback"], exact=False)


# hmc objectives of the Philox parity cases.  A parity tolerance only means something where the restatement's OWN rounding
# stays well inside it, so the cases were chosen on the CPU from the restatement alone (tools/sample_sensitivity.py: the
# run twice, once with every objective and gradient value moved at random by one unit in the last place; 200 chains,
# maxiter 30, nleap 10, stepsize 0.01, the five objectives of the reference fixtures, ndim 3 / 8 with finite differences,
# 3 / 8 / 64 analytic).  Largest deviation over those shapes, as a share of the search range / relative in funall:
#   sphere 1.9e-12 / 1.0e-11, griewank 2.6e-13 / 4.0e-12, styblinski_tang 2.0e-10 / 1.6e-9  -- three orders inside 1e-6;
#   rastrigin 1.6e-5 / 1.4e-3, ackley 4.8e-6 / 2.8e-5 -- from a random start these trajectories amplify a last-bit
#   difference (finite differences divide it by h = 1e-4, and rastrigin's curvature puts the leap-frog step near its
#   stability limit) beyond the tolerance within 30 samples, so a comparison at 1e-6 would test the rounding, not the
#   kernel.  They stay covered by the reference fixtures (hmc_rastrigin, hmc_ackley), whose margin was measured likewise.
HMC_WELL_CONDITIONED = ("sphere", "griewank", "styblinski_tang")


def philox_cases():
    out = []
    k = 0
    for ndim in (3, 8, 128, 2048):
        for chains in (1, 7, 1000):
            for return_all in (True, False):
                maxiter = 50 if ndim <= 128 else 12
                perc = (1.0, 0.5, 0.3)[k % 3]  # (0.3: blocks that do not divide ndim -- the last one is shorter)
                out.append(("mcmc", ALL[k % 7], ndim, chains, return_all,
                            {"maxiter": maxiter, "stepsize": 0.05, "perc": perc}))
                k += 1
    for ndim, jacs in ((3, (None, "analytic")), (8, (None, "analytic")), (64, ("analytic",))):
        for jac in jacs:
            for chains in (1, 7, 1000):
                for return_all in (True, False):
                    name = HMC_WELL_CONDITIONED[k % 3]
                    out.append(("hmc", name, ndim, chains, return_all,
                                {"maxiter": 30, "nleap": 10, "stepsize": 0.01, "jac": jac}))
                    k += 1
    return out


@pytest.mark.parametrize("method,objective,ndim,chains,return_all,options", philox_cases(),
                         ids=lambda v: "-".join(f"{k}={w}" for k, w in v.items()) if isinstance(v, dict) else str(v))
def test_parity_with_the_restatement_philox(sa, method, objective, ndim, chains, return_all, options):
    bounds = [[-5.12, 5.12]] * ndim
    opts = dict(options, seed=1234 + ndim + chains, rng="philox", chains=chains, return_all=return_all)
    with np.errstate(all="ignore"):
        want = _sample_oracle.sample(objective, bounds, method=method, options=dict(opts))
    got = sa.sample.sample(getattr(sa.factory, objective), bounds, method=method, options=dict(opts, backend="hip"))
    assert got.nit == want.nit
    if chains > 1:
        assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert got.accept_ratio == want.accept_ratio
    if method == "hmc":
        assert got.nfev == want.nfev
    if return_all:
        assert got.xall.shape == ((chains, opts["maxiter"], ndim) if chains > 1 else (opts["maxiter"], ndim))
        assert got.funall.shape == got.xall.shape[:-1]
        with np.errstate(all="ignore"):
            print("max |dx| / range", np.nanmax(np.abs(got.xall - want.xall)) / SPAN, "max rel df",
                  np.nanmax(np.abs(got.funall - want.funall) / np.abs(want.funall)))
        assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
    else:
        assert "xall" not in got and "funall" not in got
    assert close_samples(got.x, want.x) and close_values(got.fun, want.fun)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_reject_keeps_the_samples_in_the_box(sa, method):
    """constraints="Reject" as documented: a proposal outside [lower, upper] is rejected, without an acceptance draw.
    Steps large enough that some proposals leave the box."""
    ndim, chains = 8, 64
    bounds = [[-5.12, 5.12]] * ndim
    opts = {"maxiter": 50, "seed": 77, "rng": "philox", "chains": chains, "constraints": "Reject"}
    opts.update({"stepsize": 0.5} if method == "mcmc" else {"stepsize": 0.2, "nleap": 5, "jac": "analytic"})
    with np.errstate(all="ignore"):
        want = _sample_oracle.sample("sphere", bounds, method=method, options=dict(opts))
    got = sa.sample.sample(sa.factory.sphere, bounds, method=method, options=dict(opts, backend="hip"))
    total = chains * (opts["maxiter"] - 1)
    print(method, "rejected as infeasible:", got.nreject, "of", total)
    assert got.nreject > 0 and got.nreject == total - int(want.nfeas.sum())
    assert np.all(got.xall >= -5.12) and np.all(got.xall <= 5.12)
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_a_chain_does_not_depend_on_the_launch(sa, method):
    """Chain 5 is chain 5 whatever the number of chains (launch geometry), and a run cut into one launch per sample
    (callback) is the run in one launch -- both bit for bit."""
    bounds = [[-5.12, 5.12]] * 8
    opts = {"maxiter": 40, "seed": 5, "rng": "philox", "backend": "hip"}
    fun = sa.factory.rastrigin
    few = sa.sample.sample(fun, bounds, method=method, options=dict(opts, chains=7))
    many = sa.sample.sample(fun, bounds, method=method, options=dict(opts, chains=1000))
    assert np.array_equal(few.xall[5], many.xall[5]) and np.array_equal(few.funall[5], many.funall[5])
    assert few.accept_ratios[5] == many.accept_ratios[5]
    seen = []
    cut = sa.sample.sample(fun, bounds, method=method, options=dict(opts, chains=7),
                           callback=lambda xk, state: seen.append(np.array(xk, copy=True)))
    assert len(seen) == 40 and np.array_equal(np.stack(seen, axis=1), few.xall)
    assert np.array_equal(cut.xall, few.xall) and np.array_equal(cut.funall, few.funall)
    assert np.array_equal(cut.x, few.x) and cut.fun == few.fun and cut.accept_ratio == few.accept_ratio
    if method == "hmc":
        assert cut.nfev == few.nfev


@pytest.mark.parametrize("objective", ALL)
def test_analytic_gradients(sa, objective):
    """The kernels' closed-form gradients (sx_sample_gradient runs the hmc kernel's device functions) against the closed
    forms in numpy (tests/_sample_oracle.py GRADIENTS, themselves checked against central differences in
    test_sample_host.py), at random points, to 1e-12 of the gradient's norm."""
    import torch

    from stochopy_amd import _device, _lib

    ctx = _device.Context()
    rs = np.random.RandomState(11)
    for n in (5, 64, 200):
        X = rs.uniform(-5.0, 5.0, (33, n))
        with torch.cuda.stream(ctx.stream):
            dX = ctx.upload(X)
            dG = ctx.empty((33, n))
            _lib.check(ctx.L.sx_sample_gradient(_lib.FUN_IDS[objective], _device.ptr(dX), 33, n, _device.ptr(dG),
                                                ctx.stream_ptr), "sx_sample_gradient")
            G = dG.cpu().numpy()
        want = _sample_oracle.GRADIENTS[objective](X)
        err = np.linalg.norm(G - want, axis=1) / np.linalg.norm(want, axis=1)
        print(objective, n, "max relative error", err.max())
        assert np.all(err <= 1e-12)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_samples_the_right_distribution(sa, method):
    """Sphere, ndim = 4, x0 = 0: the target exp(-f) is N(0, I/2), the box ends 7 standard deviations out.  The last
    samples of 4096 independent chains: each component's mean has standard deviation sqrt(0.5 / C), each sample variance
    0.5 sqrt(2 / (C - 1)); all eight statistics within 5 of their standard deviations."""
    C, ndim = 4096, 4
    opts = {"seed": 2024, "rng": "philox", "chains": C, "backend": "hip"}
    opts.update({"maxiter": 400, "stepsize": 0.1} if method == "mcmc" else {"maxiter": 200, "jac": "analytic"})
    res = sa.sample.sample(sa.factory.sphere, [[-5.12, 5.12]] * ndim, x0=np.zeros(ndim), method=method, options=opts)
    last = res.xall[:, -1, :]
    mean_dev = last.mean(axis=0) / np.sqrt(0.5 / C)
    var_dev = (last.var(axis=0, ddof=1) - 0.5) / (0.5 * np.sqrt(2.0 / (C - 1)))
    print(method, "means / sd", mean_dev, "variances / sd", var_dev, "accept_ratio", res.accept_ratio)
    assert np.all(np.abs(mean_dev) <= 5.0) and np.all(np.abs(var_dev) <= 5.0)


def test_hmc_survives_non_finite_values(sa):
    """Rosenbrock with the fixtures' hmc settings overflows to NaN in the reference itself: the run finishes and accepts
    what the restatement accepts."""
    bounds = [[-5.12, 5.12]] * 8
    opts = {"maxiter": 200, "nleap": 10, "stepsize": 0.01, "seed": 204}
    saved = np.random.get_state()
    try:
        with np.errstate(all="ignore"):
            want = _sample_oracle.sample("rosenbrock", bounds, method="hmc", options=dict(opts, rng="numpy-legacy"))
        got = sa.sample.sample(sa.factory.rosenbrock, bounds, method="hmc",
                               options=dict(opts, backend="hip", rng="numpy-legacy"))
    finally:
        np.random.set_state(saved)
    print("accept_ratio", got.accept_ratio, want.accept_ratio, "NaN samples", int(np.isnan(got.funall).sum()),
          int(np.isnan(want.funall).sum()))
    assert got.nit == 200 and got.accept_ratio == want.accept_ratio and got.nfev == want.nfev


def test_hmc_finite_differences_on_the_longest_row(sa):
    """ndim = 2 048 with finite differences: the one chain of a wave needs 82 KB of LDS (five rows), more than the default
    limit of a workgroup -- the launch raises the kernel's limit.  Two samples, one leap-frog step, against the restatement."""
    ndim = 2048
    bounds = [[-5.12, 5.12]] * ndim
    opts = {"maxiter": 3, "nleap": 1, "stepsize": 0.001, "seed": 8, "rng": "philox", "chains": 3}
    with np.errstate(all="ignore"):
        want = _sample_oracle.sample("sphere", bounds, method="hmc", options=dict(opts))
    got = sa.sample.sample(sa.factory.sphere, bounds, method="hmc", options=dict(opts, backend="hip"))
    assert got.nfev == want.nfev == 3 * (1 + 2 * (3 * 2 * ndim + 2))
    assert np.array_equal(got.accept_ratios, want.accept_ratios)
    print("max |dx| / range", np.abs(got.xall - want.xall).max() / SPAN)
    assert close_samples(got.xall, want.xall) and close_values(got.funall, want.funall)
