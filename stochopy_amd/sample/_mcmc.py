"""Metropolis-Hastings (reference: stochopy/sample/mcmc/_mcmc.py)."""
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
    stepsize=0.1,
    perc=1.0,
    seed=None,
    constraints=None,
    return_all=True,
    callback=None,
    chains=1,
    rng="numpy-legacy",
    backend="hip",
):
    """Sample the variable space with the Metropolis-Hastings algorithm (``mcmc/_mcmc.py:13-161``), ``chains``
    independent chains in one kernel.

    Arguments, defaults and results are the reference's.  Sample ``i`` perturbs one block of
    ``k = max(1, int(perc * ndim))`` consecutive variables with ``randn(k) * stepsize * 0.5 * (upper - lower)``,
    the blocks taking turns from variable 0; ``x`` / ``fun`` are the best among the ACCEPTED samples (``fun`` is
    ``inf`` and ``x`` the first sample when nothing was accepted).  ``chains``, ``rng``, ``backend`` and a
    ``factory.batched`` objective (``fun(X, *args)`` on the ``(chains, ndim)`` device tensor, ``rng="philox"``):
    see ``stochopy_amd.sample.sample``.

    Where the reference is not well defined:

    - ``constraints="Reject"``: the reference's feasibility helper returns ``None`` for it, so every proposal is
      rejected.  Here it does what the documentation says: a proposal outside ``[lower, upper]`` is rejected, without
      an acceptance draw.  The draw sequence then depends on the data, so it needs ``rng="philox"``.
    - a ``k`` that does not divide ``ndim``: the reference raises a broadcasting error on the last block.  Here the
      last block is the shorter one.
    """
    run = _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                        backend)
    if not 0.0 <= perc <= 1.0:
        raise ValueError()
    run.method = _lib.SX_SAMPLE_MCMC
    run.k = max(1, int(perc * run.ndim))
    return _chains.run(run)


register("mcmc", sample)
