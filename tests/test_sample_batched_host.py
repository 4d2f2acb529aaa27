"""Samplers with a caller's own device objective (factory.batched), host side (no GPU): the argument checks raise -- and
accept -- before a device is needed, and the chunking of the finite differences' stacked rows."""
import numpy as np
import pytest

import stochopy_amd as sa
from stochopy_amd import _lib
from stochopy_amd.sample import _chains

B = [[-1.0, 1.0]] * 4


def user_fun(X, *args):
    return (X * X).sum(1)


def user_grad(X, *args):
    return 2.0 * X


FUN = sa.factory.batched(user_fun)
GRAD = sa.factory.batched(user_grad)


def setup(fun=FUN, bounds=B, x0=None, args=(), maxiter=10, stepsize=0.1, seed=1, constraints=None, return_all=True,
          callback=None, chains=1, rng="philox", backend="hip", nleap=None):
    return _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                         backend, nleap=nleap)


def test_a_batched_objective_passes_setup_with_philox_and_a_seed():
    s = setup(args=(1.0, 2.0), chains=5)
    assert s.external is not None and s.external.fun is user_fun and s.external.args == (1.0, 2.0)
    assert s.gradient is None and s.rng == "philox" and s.chains == 5 and s.ndim == 4
    assert setup(sa.factory.sphere).external is None  # a factory objective stays on the fused path
    s = setup(constraints="Reject", return_all=False, x0=np.zeros((3, 4)), chains=3)
    assert s.reject and not s.return_all and s.x0.shape == (3, 4)


def test_a_batched_objective_needs_philox():
    with pytest.raises(TypeError, match="philox"):
        setup(rng="numpy-legacy")
    for method in ("mcmc", "hmc"):
        with pytest.raises(TypeError, match="philox"):
            sa.sample.sample(FUN, B, method=method)  # numpy-legacy is the default
        with pytest.raises(TypeError, match="philox"):
            sa.sample.sample(FUN, B, method=method, options={"seed": 1, "chains": 4})
    with pytest.raises(ValueError):
        setup(seed=None)  # Philox draws need a seed
    with pytest.raises(TypeError, match="factory"):
        setup(fun=user_fun)  # a plain callable is not a device objective
    with pytest.raises(TypeError):
        setup(sa.factory.sphere, args=(1.0,))  # factory objectives take no args


def test_what_failed_before_still_fails():
    with pytest.raises(ValueError):
        setup(x0=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        setup(x0=np.zeros((3, 4)), chains=2)
    with pytest.raises(ValueError):
        setup(chains=0)
    with pytest.raises(ValueError):
        setup(chains=2.5)
    with pytest.raises(ValueError):
        setup(bounds=[[-1.0, 1.0]] * (_lib.wide_from() + 1))
    with pytest.raises(ValueError):
        setup(maxiter=0)
    with pytest.raises(ValueError):
        setup(constraints="Shrink")
    with pytest.raises(ValueError):
        setup(backend="cpu")
    with pytest.raises(ValueError):
        setup(nleap=0)
    with pytest.raises(ValueError):
        setup(stepsize=[0.1, 0.1])
    for method in ("mcmc", "hmc"):
        with pytest.raises(ValueError):
            sa.sample.sample(FUN, B, x0=[0.0, 0.0, 0.0], method=method, options={"rng": "philox", "seed": 1})
        with pytest.raises(ValueError):
            sa.sample.sample(FUN, B, method=method, options={"rng": "philox", "seed": 1, "chains": 0})
    with pytest.raises(ValueError):
        sa.sample.sample(FUN, B, method="mcmc", options={"rng": "philox", "seed": 1, "perc": 1.5})


def hmc_checks(monkeypatch, fun, jac, **options):
    """sample.hmc up to the point where it would touch the device: the checked run, as _chains.run receives it."""
    seen = []
    monkeypatch.setattr(_chains, "run", lambda s: seen.append(s) or "ran")
    opts = dict({"rng": "philox", "seed": 1, "chains": 3, "jac": jac}, **options)
    assert sa.sample.sample(fun, B, method="hmc", options=opts) == "ran"
    return seen[0]


def test_the_forms_of_jac_that_are_accepted(monkeypatch):
    s = hmc_checks(monkeypatch, FUN, None, finite_diff_abs_step=1e-3)
    assert s.gradient is None and s.jac == _lib.SX_JAC_FINITE_DIFF and s.fd_step == 1e-3
    s = hmc_checks(monkeypatch, FUN, GRAD)
    assert isinstance(s.gradient, _chains.Gradient) and s.gradient.fun is user_grad and s.jac == _lib.SX_JAC_ANALYTIC
    s = hmc_checks(monkeypatch, FUN, "autograd")
    assert isinstance(s.gradient, _chains.AutogradGradient) and s.gradient.external is s.external
    assert s.jac == _lib.SX_JAC_ANALYTIC  # (no finite-difference calls in nfev)
    for jac, want in ((None, _lib.SX_JAC_FINITE_DIFF), ("analytic", _lib.SX_JAC_ANALYTIC)):
        s = hmc_checks(monkeypatch, sa.factory.sphere, jac)
        assert s.external is None and s.gradient is None and s.jac == want


def test_args_reach_the_gradient(monkeypatch):
    seen = []
    monkeypatch.setattr(_chains, "run", lambda s: seen.append(s))
    sa.sample.sample(FUN, B, args=(3.0,), method="hmc", options={"rng": "philox", "seed": 1, "jac": GRAD})
    assert seen[0].external.args == (3.0,) and seen[0].gradient.args == (3.0,)


def test_the_forms_of_jac_that_are_refused():
    def raises(fun, jac, match=None):
        with pytest.raises(TypeError, match=match):
            sa.sample.sample(fun, B, method="hmc", options={"rng": "philox", "seed": 1, "jac": jac})

    raises(FUN, "analytic", match="autograd")  # names the two alternatives
    raises(FUN, "analytic", match=r"factory\.batched\(g\)")
    raises(FUN, user_grad)  # a plain callable
    raises(FUN, "numeric")
    raises(sa.factory.sphere, GRAD)
    raises(sa.factory.sphere, "autograd")
    raises(sa.factory.sphere, user_grad)
    raises(sa.factory.sphere, "numeric")
    raises(sa.factory.sphere, np.zeros(4))


@pytest.mark.parametrize("chains,ndim,stack_bytes,want", [
    (7, 8, 2 * 7 * 8 * 8 * 3, [3, 3, 2]),          # three axes fit: 3 + 3 + 2
    (7, 8, 2 * 7 * 8 * 8 * 3 + 100, [3, 3, 2]),    # (not a multiple of an axis' bytes)
    (7, 8, 1, [1] * 8),                            # nothing fits: one axis per chunk, never 0
    (7, 8, 2 * 7 * 8 * 8 - 1, [1] * 8),
    (7, 8, 256 << 20, [8]),                        # everything fits: the chunk is not longer than the row
    (1, 1, 256 << 20, [1]),
    (16384, 64, 256 << 20, [16, 16, 16, 16]),      # 16 MiB per axis
    (16384, 2048, 256 << 20, [1] * 2048),          # 512 MiB per axis: more than the limit, still one axis
    (1000, 130, 256 << 20, [129, 1]),              # a shorter last chunk
    (5, 10, 2 * 5 * 10 * 8 * 4, [4, 4, 2]),
])
def test_finite_difference_chunks(monkeypatch, chains, ndim, stack_bytes, want):
    monkeypatch.setattr(_chains, "FD_STACK_BYTES", stack_bytes)
    chunk = _chains.fd_axes_per_chunk(chains, ndim)
    assert 1 <= chunk <= ndim
    got = [min(chunk, ndim - axis0) for axis0 in range(0, ndim, chunk)]
    assert got == want and sum(got) == ndim
    assert chunk == 1 or 2 * chunk * chains * ndim * 8 <= stack_bytes
