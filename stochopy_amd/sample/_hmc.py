"""Hamiltonian (hybrid) Monte-Carlo (reference: stochopy/sample/hmc/_hmc.py)."""
from .. import _lib
from . import _chains
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
      gradient at the origin is taken as 0, and griewank's needs every cosine factor to be non-zero).  Anything else
      raises ``TypeError``.
    - ``constraints="Reject"``: the reference's feasibility helper returns ``None`` for it, so every proposal is
      rejected.  Here a trajectory that ends outside ``[lower, upper]`` is rejected, without an acceptance draw.  The
      draw sequence then depends on the data, so it needs ``rng="philox"``.
    """
    run = _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                        backend, nleap=nleap)
    if not (jac is None or jac == "analytic"):
        raise TypeError('jac is None (finite differences) or "analytic" (the factory objective\'s closed-form gradient)')
    run.method = _lib.SX_SAMPLE_HMC
    run.nleap = int(nleap)
    run.jac = _lib.SX_JAC_FINITE_DIFF if jac is None else _lib.SX_JAC_ANALYTIC
    run.fd_step = float(finite_diff_abs_step)
    return _chains.run(run)


register("hmc", sample)
