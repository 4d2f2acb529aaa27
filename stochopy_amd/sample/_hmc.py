"""Hamiltonian (hybrid) Monte-Carlo (reference: stochopy/sample/hmc/_hmc.py)."""
from .. import _lib
from ..factory.benchmark import batched
from . import _adapt, _chains
from ._helpers import register

__all__ = ["sample"]


def sample(
    fun,
    bounds,
    x0=None,
    args=(),
    maxiter=100,
    nleap=10,
    stepsize=0.01,
    seed=None,
    jac=None,
    finite_diff_abs_step=1.0e-4,
    constraints=None,
    return_all=True,
    callback=None,
    chains=1,
    rng="numpy-legacy",
    backend="hip",
    temperatures=None,
    swap_every=None,
    warmup=0,
    target_accept=None,
    burn=None,
    thin=1,
    metric=None,
):
    """Sample the variable space with Hamiltonian Monte-Carlo (``hmc/_hmc.py:13-200``), ``chains`` independent
    chains in one kernel.

    Arguments, defaults and results are the reference's.  Per sample: a momentum ``randn(ndim)``, then a half
    momentum step, a position step, ``nleap`` times (momentum step, position step) and a half momentum step --
    ``nleap + 2`` gradients; ``x`` / ``fun`` are the ``argmin`` over ``funall``; ``nfev`` counts every objective call
    the reference would make, the finite differences' included (summed over the chains).  ``chains``, ``rng``,
    ``backend``: see ``stochopy_amd.sample.sample``.

    Where the reference is not well defined:

    - ``jac``: the reference recurses without end for a callable.  Here ``jac`` is ``None`` (2-point finite
      differences with ``finite_diff_abs_step``, as the reference, perturbing and restoring the components in place)
      or the string ``"analytic"`` (the closed-form gradient of the factory objective, computed in the kernel; ackley's
      gradient at the origin is taken as 0, and griewank's needs every cosine factor to be non-zero).  With a
      ``factory.batched`` objective (see ``stochopy_amd.sample.sample``) ``jac`` is ``None`` (the same finite
      differences, the perturbed rows of several axes stacked into one call of ``fun``; ``nfev`` counts them),
      ``factory.batched(g)`` (``g(X, *args)`` returns the ``(chains, ndim)`` gradient tensor on the same device) or
      ``"autograd"`` (``torch.autograd.grad(fun(X).sum(), X)``: rows are independent, so that is each chain's own
      gradient); ``"analytic"`` is for factory objectives only.  Anything else raises ``TypeError``.
    - ``constraints="Reject"``: the reference's feasibility helper returns ``None`` for it, so every proposal is
      rejected.  Here a trajectory that ends outside ``[lower, upper]`` is rejected, without an acceptance draw.  The
      draw sequence then depends on the data, so it needs ``rng="philox"``.
    - ``temperatures`` / ``swap_every`` (parallel tempering, see ``sample.mcmc``) are refused: tempering the potential
      and its gradient is not built.

    ``warmup`` / ``target_accept`` / ``burn`` / ``thin`` (``rng="philox"``): per-chain step-size adaptation in a warm-up,
    burn-in and thinning, as ``sample.mcmc`` describes them; the multiplier scales the momentum and the position steps
    alike, the default ``target_accept`` is 0.65, and a trajectory whose ``d`` is NaN counts as rejected in the
    adaptation (it shrinks the step) while the decision itself stays what it is.  They work with every ``jac``.

    ``metric="diag"`` (``warmup >= 20``, ``rng="philox"``): per-axis scales learnt in the warm-up, as ``sample.mcmc``
    describes them.  The momentum and the position steps read ``s_c * m_c[e] * stepsize[e]``; the momenta stay ``randn(ndim)``
    and the kinetic energy ``0.5 sum p^2`` -- leap-frog in coordinates rescaled per axis, which is HMC with the diagonal mass
    matrix ``1 / m^2``, so the decision rule is untouched.  It works with every ``jac``.
    """
    if temperatures is not None or swap_every is not None:
        _adapt.refuse_with_temperatures(warmup, target_accept, burn, thin)
        _adapt.check_metric(metric, with_temperatures=True)
        raise ValueError('temperatures / swap_every (parallel tempering) are served by method="mcmc" only')
    run = _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                        backend, nleap=nleap)
    external = run.external is not None
    own_gradient = isinstance(jac, batched) or (isinstance(jac, str) and jac == "autograd")
    if own_gradient and not external:
        raise TypeError('jac=factory.batched(g) and jac="autograd" go with a factory.batched objective; a factory objective '
                        'takes jac=None or "analytic"')
    if isinstance(jac, str) and jac == "analytic" and external:
        raise TypeError('jac="analytic" is the closed form of a factory objective; with a factory.batched objective give '
                        'jac=factory.batched(g) (your own gradient) or jac="autograd", or None for finite differences')
    if not (jac is None or own_gradient or (isinstance(jac, str) and jac == "analytic")):
        raise TypeError('jac is None (finite differences), "analytic" (a factory objective\'s closed-form gradient), or, with '
                        'a factory.batched objective, factory.batched(g) or "autograd"')
    run.method = _lib.SX_SAMPLE_HMC
    run.nleap = int(nleap)
    run.jac = _lib.SX_JAC_FINITE_DIFF if jac is None else _lib.SX_JAC_ANALYTIC
    if isinstance(jac, batched):
        run.gradient = _chains.Gradient(jac, args)
    elif own_gradient:
        run.gradient = _chains.AutogradGradient(run.external)
    run.fd_step = float(finite_diff_abs_step)
    run.adapt = _adapt.check(warmup, target_accept, burn, thin, rng, run.maxiter, 0.65, metric)
    return _chains.run(run)


register("hmc", sample)
