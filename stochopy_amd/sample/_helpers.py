"""API surface of the reference's sampling half.

Reference: stochopy/sample/_helpers.py:8-88 (``SampleResult``, ``register``, ``sample``) and stochopy/_common.py
(``BaseResult``: dict with attribute access whose repr sorts keys and hides xall / funall).
"""
from ..optimize._helpers import OptimizeResult

__all__ = ["SampleResult", "sample", "register"]

_sampler_map = {}
# this backend's own methods (no counterpart in the reference): consulted after _sampler_map
_own_sampler_map = {}


class SampleResult(OptimizeResult):
    """Sampling result: keys x, fun, nit, accept_ratio (+ nfev for hmc, xall / funall with ``return_all``, and
    accept_ratios with more than one chain; with ``temperatures``: accept_ratios per ladder and rung, temperatures and
    swap_ratios; with ``warmup``: stepsizes, accept_ratios_sampling and warmup; with ``metric``: metric and metric_windows)."""


def register(name, sample):
    """Register a sampler under ``method=name`` (reference _helpers.py:36-38)."""
    _sampler_map[name] = sample


def register_own(name, sample):
    """Register one of this backend's own samplers under ``method=name``."""
    _own_sampler_map[name] = sample


def sample(fun, bounds, x0=None, args=(), method="mcmc", options=None, callback=None):
    """Sample the variable space of ``fun`` on the GPU.

    Same signature and dispatch as the reference (``_helpers.py:41-88``): ``options`` is splatted into the
    per-method function, ``method`` is ``"mcmc"`` or ``"hmc"``.  ``fun`` is one of the ``stochopy_amd.factory``
    handles (fused into the chain kernels), or the caller's own device objective tagged with ``factory.batched``:
    ``fun(X, *args)`` maps the ``(chains, ndim)`` float64 ROCm tensor of proposals to the ``(chains,)`` tensor of
    values on the same device (``args`` is passed through; needs ``rng="philox"``).  A sample then is propose kernel ->
    ``fun`` -> decide kernel, launched one by one: same draws, same arithmetic, same results for the same values, a
    few launches per sample slower.  A plain Python callable raises ``TypeError``.  Options added by this backend:

    - ``chains`` (int >= 1, default 1): independent chains, each resident in one kernel for the whole run.  With
      ``chains = C > 1`` the result's ``xall`` is ``(C, maxiter, ndim)``, ``funall`` ``(C, maxiter)``, ``x`` / ``fun``
      the best over all chains by the method's own rule applied per chain, ``accept_ratio`` the overall ratio and
      ``accept_ratios`` one per chain; ``x0`` may be ``(ndim,)`` (shared) or ``(C, ndim)``; the callback's ``xk`` is
      ``(C, ndim)``.
    - ``rng``: ``"numpy-legacy"`` (default) replays the reference's own global MT19937 stream and needs
      ``chains == 1``; ``"philox"`` makes every draw inside the kernel and serves any ``chains``.
    - ``backend="hip"``: accepted, the only backend.
    - ``temperatures`` / ``swap_every`` (``method="mcmc"``, ``rng="philox"``): parallel tempering.  ``temperatures`` is a
      ladder ``1 = T_0 < T_1 < ... < T_{K-1}`` and ``chains = C`` the number of ladders of K replicas; neighbouring rungs
      exchange their states every ``swap_every`` samples (default 1).  The result holds the cold rungs (``xall``,
      ``funall``, ``x``, ``fun``, ``accept_ratio``), ``accept_ratios (C, K)``, ``temperatures (K,)`` and
      ``swap_ratios (C, K-1)``; the callback's ``xk`` is the ``(C, ndim)`` cold states.  See ``sample.mcmc``.

    - ``warmup`` / ``target_accept`` / ``burn`` / ``thin`` (``rng="philox"``; not with ``temperatures``): ``warmup=W``
      adapts a per-chain multiplier of ``stepsize`` over samples 1 ... W (dual averaging towards ``target_accept``) and
      freezes it; ``xall`` / ``funall`` hold samples ``burn, burn + thin, ...`` only (``burn`` defaults to ``warmup``).
      The result gains ``stepsizes``, ``accept_ratios_sampling`` and ``warmup``.  See ``sample.mcmc``.
    - ``metric="diag"`` (``warmup >= 20``, ``rng="philox"``; not with ``temperatures``): every chain also learns one scale
      per axis in windows of the warm-up, from the variance of its own samples, for targets whose axes differ in width.
      The result gains ``metric`` and ``metric_windows``.  See ``sample.mcmc``.

    ``method="ensemble"`` (this backend's own; ``rng="philox"``): the affine-invariant ensemble sampler -- ``chains``
    ensembles of ``walkers`` walkers, no step size, no gradient; ``moves`` adds the differential-evolution and snooker
    moves for targets with separated modes, ``burn`` / ``thin`` choose the samples recorded.  See ``sample.ensemble``.

    ``method="smc"`` (this backend's own; ``rng="philox"``): tempered sequential Monte Carlo -- ``chains`` populations of
    ``particles`` particles walked from the uniform prior on ``bounds`` to ``exp(-fun)`` through a ladder of inverse
    temperatures the sampler chooses itself, ``steps`` Metropolis steps per particle and stage.  It returns the final particles
    and ``log_evidence``, the log of the integral of ``exp(-fun)`` over the box divided by the box's volume, which no chain or
    ensemble can give, and finds the weights of separated modes from a cold start.  See ``sample.smc``.

    See ``sample.mcmc`` / ``sample.hmc`` for where this backend departs from the reference.
    """
    options = options if options else {}
    if method not in _sampler_map and method in _own_sampler_map:
        sampler = _own_sampler_map[method]
    else:
        sampler = _sampler_map[method]

    return sampler(fun=fun, bounds=bounds, x0=x0, args=args, callback=callback, **options)
