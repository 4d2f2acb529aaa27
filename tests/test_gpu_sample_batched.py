"""GPU: stochopy_amd.sample with a caller's own device objective (factory.batched; csrc/sx_sample_unfused.hip: a sample is
propose -> objective -> decide, hmc with nleap + 2 rounds of gradient -> leap in between).  With bit-identical objective and
gradient values the run must be the fused run (csrc/sx_sample.hip), bit for bit; with an objective written in torch it must
be the numpy restatement's run (tests/_sample_oracle.py) within the project's parity tolerances (test_gpu_sample.py: 1e-6 of
the search range for samples, 1e-6 relative for values, counts exact) and sample the distribution it is given."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_oracle  # noqa: E402
from oracle import objectives  # noqa: E402

pytestmark = pytest.mark.gpu

SPAN = 10.24


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def device_objective(sa, name):
    """A "user" objective that happens to return the fused kernels' values: sx_eval on the stream it is called on
    (the pattern of test_gpu_external.py device_objective)."""
    import torch

    from stochopy_amd import _lib

    L, fid = _lib.lib(), _lib.FUN_IDS[name]

    def fun(X):
        P, n = X.shape
        f = torch.empty((P,), dtype=torch.float64, device=X.device)
        X = X.contiguous()
        assert L.sx_eval(fid, X.data_ptr(), P, n, n, None, None, f.data_ptr(), None, None,
                         C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        return f

    fun.__name__ = "device_" + name
    return sa.factory.batched(fun)


def device_gradient(sa, name):
    """A "user" gradient that happens to return the fused hmc kernel's closed form: sx_sample_gradient."""
    import torch

    from stochopy_amd import _lib

    L, fid = _lib.lib(), _lib.FUN_IDS[name]

    def grad(X):
        P, n = X.shape
        G = torch.empty((P, n), dtype=torch.float64, device=X.device)
        X = X.contiguous()
        assert L.sx_sample_gradient(fid, X.data_ptr(), P, n, G.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        return G

    grad.__name__ = "device_grad_" + name
    return sa.factory.batched(grad)


def assert_same_run(ext, fused, chains, return_all):
    assert ext.nit == fused.nit
    assert ("accept_ratios" in fused) == (chains > 1) and ("xall" in fused) == return_all
    for key in ("x", "fun", "accept_ratio"):
        assert np.array_equal(ext[key], fused[key]), key
    for key in ("accept_ratios", "nfev", "nreject", "xall", "funall"):
        assert (key in ext) == (key in fused), key
        if key in fused:
            assert np.array_equal(ext[key], fused[key]), key
    if return_all:
        assert np.all(np.isfinite(fused.funall))  # (array_equal means something: no NaN)


def both(sa, method, objective, ndim, opts, ext_jac=None, callback=None):
    bounds = [[-5.12, 5.12]] * ndim
    o = dict(opts, rng="philox", backend="hip")
    fused = sa.sample.sample(getattr(sa.factory, objective), bounds, method=method, options=dict(o))
    if method == "hmc" and o.get("jac") == "analytic":
        o["jac"] = ext_jac if ext_jac is not None else device_gradient(sa, objective)
    ext = sa.sample.sample(device_objective(sa, objective), bounds, method=method, options=o, callback=callback)
    return ext, fused


# ---- test 1: bit for bit with the fused run -----------------------------------------------------------------------------
# ndim 3 / 130: not a multiple of the 16 / 64 lanes of a row; 130 / 200: two elements of a lane share a Box-Muller call;
# 2 048: the longest row; chains 1 / 7 / 1000: a partial last workgroup (16 chains per workgroup up to ndim 64, 8 from
# ndim 129); perc 0.5 / 0.3: blocks of int(perc * ndim) variables, the last one shorter when they do not divide ndim
MCMC = [
    ("sphere", 3, 1, 1.0, True, 30),
    ("rastrigin", 3, 7, 0.5, False, 30),
    ("styblinski_tang", 3, 1000, 0.3, True, 30),
    ("styblinski_tang", 130, 7, 0.3, True, 30),
    ("rastrigin", 130, 1000, 1.0, False, 30),
    ("sphere", 200, 7, 0.5, True, 30),
    ("styblinski_tang", 200, 1000, 0.3, False, 30),
    ("rastrigin", 2048, 1, 0.3, True, 12),
    ("sphere", 2048, 7, 1.0, True, 12),
    ("styblinski_tang", 2048, 1000, 0.5, False, 8),
]


@pytest.mark.parametrize("objective,ndim,chains,perc,return_all,maxiter", MCMC)
def test_mcmc_is_the_fused_run(sa, objective, ndim, chains, perc, return_all, maxiter):
    opts = {"maxiter": maxiter, "stepsize": 0.05, "perc": perc, "seed": 100 + ndim + chains, "chains": chains,
            "return_all": return_all}
    ext, fused = both(sa, "mcmc", objective, ndim, opts)
    assert_same_run(ext, fused, chains, return_all)
    if ndim <= 200:  # (both outcomes of the decision occur; checked with the restatement)
        assert 0.0 < fused.accept_ratio < 1.0


HMC = [
    ("sphere", 3, 1, True),
    ("rastrigin", 8, 7, False),
    ("styblinski_tang", 64, 1000, True),
    ("sphere", 200, 7, True),
    ("rastrigin", 200, 1000, False),
]


@pytest.mark.parametrize("objective,ndim,chains,return_all", HMC)
def test_hmc_with_a_batched_gradient_is_the_fused_analytic_run(sa, objective, ndim, chains, return_all):
    opts = {"maxiter": 30, "nleap": 10, "stepsize": 0.01, "jac": "analytic", "seed": 200 + ndim + chains, "chains": chains,
            "return_all": return_all}
    ext, fused = both(sa, "hmc", objective, ndim, opts)
    assert_same_run(ext, fused, chains, return_all)
    assert ext.nfev == chains + 2 * chains * 29  # no finite-difference calls are counted


# (objective, ndim, chains, return_all, axes per chunk or None for the default limit)
HMC_FD = [
    ("sphere", 3, 7, True, None),
    ("styblinski_tang", 8, 7, True, 3),     # the 8 axes split 3 + 3 + 2
    ("rastrigin", 8, 1000, False, 3),
    ("sphere", 8, 1, True, 1),               # one axis per call
]


@pytest.mark.parametrize("objective,ndim,chains,return_all,axes", HMC_FD)
def test_hmc_finite_differences_are_the_fused_ones(sa, monkeypatch, objective, ndim, chains, return_all, axes):
    from stochopy_amd.sample import _chains

    if axes is not None:
        monkeypatch.setattr(_chains, "FD_STACK_BYTES", 2 * chains * ndim * 8 * axes)
        assert _chains.fd_axes_per_chunk(chains, ndim) == axes
    else:
        assert _chains.fd_axes_per_chunk(chains, ndim) == ndim
    opts = {"maxiter": 30, "nleap": 10, "stepsize": 0.01, "jac": None, "seed": 300 + ndim + chains, "chains": chains,
            "return_all": return_all}
    ext, fused = both(sa, "hmc", objective, ndim, opts)
    assert_same_run(ext, fused, chains, return_all)
    assert ext.nfev == chains * (1 + 29 * 2 * ndim * 12) + 2 * chains * 29


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_reject_is_the_fused_run(sa, method):
    """constraints="Reject" with the step sizes of test_gpu_sample.py test_reject_keeps_the_samples_in_the_box: some
    proposals leave the box and are rejected without an acceptance draw."""
    opts = {"maxiter": 50, "seed": 77, "chains": 64, "constraints": "Reject", "return_all": True}
    opts.update({"stepsize": 0.5} if method == "mcmc" else {"stepsize": 0.2, "nleap": 5, "jac": "analytic"})
    ext, fused = both(sa, method, "sphere", 8, opts)
    assert_same_run(ext, fused, 64, True)
    assert ext.nreject > 0
    assert np.all(ext.xall >= -5.12) and np.all(ext.xall <= 5.12)


# ---- test 2: cut into launches ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_a_callback_does_not_change_the_run(sa, method):
    opts = {"maxiter": 20, "seed": 5, "chains": 7, "return_all": True}
    if method == "hmc":
        opts["jac"] = "analytic"
    seen, states = [], []

    def callback(xk, state):
        seen.append(np.array(xk, copy=True))
        states.append((state.nit, len(state.xall[0]), float(state.fun)))

    plain, fused = both(sa, method, "rastrigin", 8, opts)
    cut, _ = both(sa, method, "rastrigin", 8, opts, callback=callback)
    assert_same_run(plain, fused, 7, True)
    assert_same_run(cut, plain, 7, True)
    assert len(seen) == 20 and np.array_equal(np.stack(seen, axis=1), plain.xall)
    assert [s[0] for s in states] == list(range(1, 21))
    assert [s[1] for s in states] == [1] + list(range(1, 20))  # xall WITHOUT the newest sample, as the reference


# ---- tests 3 and 4: an objective the factory cannot express, written with torch ops ---------------------------------------
def gaussian_case():
    """mu, A, Sigma of the correlated Gaussian exp(-f), f(x) = 0.5 (x - mu)^T A (x - mu), ndim 4: Sigma = A^-1 has the
    eigenvalues 0.25, 0.5, 0.75, 1 on the axes of a fixed rotation (the box [-5.12, 5.12]^4 ends 4.6 standard deviations out)."""
    q, _ = np.linalg.qr(np.random.RandomState(0).randn(4, 4))
    lam = np.array([0.25, 0.5, 0.75, 1.0])
    sigma = (q * lam) @ q.T
    A = (q / lam) @ q.T
    return np.array([0.5, -0.3, 0.2, 0.1]), 0.5 * (A + A.T), sigma


def torch_gaussian(X, mu, A):
    d = X - mu
    return 0.5 * (d[:, :, None] * A[None, :, :] * d[:, None, :]).sum(dim=(1, 2))


def torch_gaussian_gradient(X, mu, A):
    return ((X - mu)[:, None, :] * A[None, :, :]).sum(dim=2)


@pytest.fixture
def gaussian(sa, monkeypatch):
    """The case's arrays on the host and on the device, and its numpy twin registered with the restatement."""
    import torch

    mu, A, sigma = gaussian_case()
    monkeypatch.setitem(objectives.OBJECTIVES, "gaussian", lambda X: 0.5 * np.einsum("ci,ij,cj->c", X - mu, A, X - mu))
    monkeypatch.setitem(_sample_oracle.GRADIENTS, "gaussian", lambda X: (X - mu) @ A)
    dev = sa._device.Context().device
    return mu, A, sigma, (torch.as_tensor(mu, device=dev), torch.as_tensor(A, device=dev))


# The tolerances mean something only where the restatement's own rounding stays far inside them.  Measured on the CPU from
# the restatement alone, the way tools/sample_sensitivity.py does (the run twice, the second time with every objective and
# gradient value moved at random by one unit in the last place; these mu, A, seeds, chains 7 and 200, maxiter 30):
#   mcmc  max |dx| / range 0       max rel df 2.2e-16   no acceptance flips
#   hmc   max |dx| / range 8.7e-17 max rel df 1.6e-15   no acceptance flips
# -- nine orders of magnitude inside 1e-6.
@pytest.mark.parametrize("chains", [7, 200])
@pytest.mark.parametrize("method,jac", [("mcmc", None), ("hmc", "batched"), ("hmc", "autograd")])
def test_a_torch_objective_against_the_restatement(sa, gaussian, method, jac, chains):
    mu, A, sigma, args = gaussian
    bounds = [[-5.12, 5.12]] * 4
    opts = {"maxiter": 30, "seed": 31 + chains, "rng": "philox", "chains": chains}
    want = _sample_oracle.sample("gaussian", bounds, method=method,
                                 options=dict(opts, jac="analytic") if method == "hmc" else dict(opts))
    if method == "hmc":
        opts["jac"] = sa.factory.batched(torch_gaussian_gradient) if jac == "batched" else "autograd"
    got = sa.sample.sample(sa.factory.batched(torch_gaussian), bounds, args=args, method=method,
                           options=dict(opts, backend="hip"))
    print("max |dx| / range", np.abs(got.xall - want.xall).max() / SPAN, "max rel df",
          np.max(np.abs(got.funall - want.funall) / np.abs(want.funall)), "accept_ratio", got.accept_ratio)
    assert got.nit == want.nit == 30
    assert np.array_equal(got.accept_ratios, want.accept_ratios) and got.accept_ratio == want.accept_ratio
    if method == "hmc":
        assert got.nfev == want.nfev
    assert got.xall.shape == (chains, 30, 4) and got.funall.shape == (chains, 30)
    assert np.allclose(got.xall, want.xall, rtol=0, atol=1e-6 * SPAN)
    assert np.allclose(got.funall, want.funall, rtol=1e-6, atol=0)
    assert np.allclose(got.x, want.x, rtol=0, atol=1e-6 * SPAN) and np.isclose(got.fun, want.fun, rtol=1e-6, atol=0)


@pytest.mark.parametrize("method", ["mcmc", "hmc"])
def test_a_torch_objective_samples_its_distribution(sa, gaussian, method):
    """The correlated Gaussian from x0 = mu, the last samples of 4096 independent chains: every component's mean within 5 of
    its standard deviation sqrt(Sigma_ii / C), every sample variance within 5 of Sigma_ii sqrt(2 / (C - 1)), the covariance
    of components 0 and 1 within 5 of sqrt((Sigma_00 Sigma_11 + Sigma_01^2) / (C - 1)).  With this seed the restatement
    (CPU) lands within 3 standard deviations on all nine: the largest are 1.53 (mcmc) and 1.29 (hmc)."""
    mu, A, sigma, args = gaussian
    Cn = 4096
    opts = {"seed": 7, "rng": "philox", "chains": Cn, "backend": "hip"}
    opts.update({"maxiter": 400, "stepsize": 0.1} if method == "mcmc" else {"maxiter": 200, "jac": "autograd"})
    res = sa.sample.sample(sa.factory.batched(torch_gaussian), [[-5.12, 5.12]] * 4, x0=mu, args=args, method=method,
                           options=opts)
    last = res.xall[:, -1, :]
    var = np.diag(sigma)
    mean_dev = (last.mean(axis=0) - mu) / np.sqrt(var / Cn)
    var_dev = (last.var(axis=0, ddof=1) - var) / (var * np.sqrt(2.0 / (Cn - 1)))
    cov_dev = (np.cov(last[:, 0], last[:, 1])[0, 1] - sigma[0, 1]) / np.sqrt((var[0] * var[1] + sigma[0, 1] ** 2) / (Cn - 1))
    print(method, "means / sd", mean_dev, "variances / sd", var_dev, "covariance / sd", cov_dev, "accept_ratio",
          res.accept_ratio)
    assert np.all(np.abs(mean_dev) <= 5.0) and np.all(np.abs(var_dev) <= 5.0) and abs(cov_dev) <= 5.0


# ---- test 5: misuse on the device ---------------------------------------------------------------------------------------
def test_misuse_raises_and_the_process_stays_usable(sa):
    import torch

    bounds = [[-5.12, 5.12]] * 4
    opts = {"maxiter": 5, "seed": 1, "rng": "philox", "chains": 6, "backend": "hip"}
    good = sa.factory.batched(lambda X: (X * X).sum(1))

    def run(fun, method="mcmc", **more):
        return sa.sample.sample(fun, bounds, method=method, options=dict(opts, **more))

    with pytest.raises(TypeError, match="expected a tensor on"):
        run(sa.factory.batched(lambda X: (X * X).sum(1).cpu()))
    with pytest.raises(TypeError, match="expected a tensor on"):
        run(sa.factory.batched(lambda X: (X * X).sum(1).cpu().numpy()))
    with pytest.raises(ValueError, match=r"expected shape \(6,\)"):
        run(sa.factory.batched(lambda X: (X * X).sum(1, keepdim=True)))
    with pytest.raises(ValueError, match=r"expected shape \(6, 4\)"):
        run(good, "hmc", jac=sa.factory.batched(lambda X: (2.0 * X).sum(1)))
    with pytest.raises(TypeError, match="expected a tensor on"):
        run(good, "hmc", jac=sa.factory.batched(lambda X: (2.0 * X).cpu()))
    with pytest.raises(ValueError, match=r"expected shape \(48,\)"):  # the finite differences' stacked rows: 2 * 4 * 6
        run(sa.factory.batched(lambda X: (X * X).sum(1)[:6] if X.shape[0] > 6 else (X * X).sum(1)), "hmc")
    for method in ("mcmc", "hmc"):
        res = run(good, method)
        assert res.nit == 5 and res.xall.shape == (6, 5, 4) and np.all(np.isfinite(res.funall))
    assert torch.cuda.is_available()
