"""Metropolis-Hastings (reference: stochopy/sample/mcmc/_mcmc.py)."""
from .. import _lib
from . import _adapt, _chains
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
    temperatures=None,
    swap_every=None,
    warmup=0,
    target_accept=None,
    burn=None,
    thin=1,
    metric=None,
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

    Parallel tempering (no counterpart in the reference; ``rng="philox"``): ``temperatures`` is a ladder
    ``1 = T_0 < T_1 < ... < T_{K-1}`` and ``chains = C`` the number of LADDERS, each of K replicas that live in one
    workgroup; ``swap_every`` (integer >= 1, default 1) is the number of samples between two exchange events.  Replica
    ``q = c K + k`` (rung k of ladder c) samples ``p^(1/T_k)`` -- the rule above with ``d = (fcur - fprop) / T_k``, draws
    keyed by q -- and after sample ``it >= 1`` with ``it % swap_every == 0`` neighbouring rungs ((0,1), (2,3), ... at odd
    events ``it // swap_every``, (1,2), (3,4), ... at even ones) exchange their states with probability
    ``min(1, exp((1/T_k - 1/T_{k+1}) (f_k - f_{k+1})))``.  The result holds the cold rungs (``T = 1``, correct samplers of
    ``p`` that visit every mode): ``xall (C, maxiter, ndim)`` / ``funall`` (squeezed for ``C = 1``), ``x`` / ``fun`` and
    ``accept_ratio`` (and ``nreject``) over the cold rungs, with an arriving state compared as an accepted sample is;
    ``accept_ratios (C, K)``, ``temperatures (K,)`` and ``swap_ratios (C, K-1)``: accepted exchanges of a pair over the
    events it took part in (0.0 where it had none).  ``x0`` is ``None`` (every replica draws its own point),
    ``(ndim,)`` (shared) or ``(C, ndim)`` (one point per ladder, shared by its rungs); the callback's ``xk`` is the
    ``(C, ndim)`` cold states.  K is at most ``sx_sample_tempered_max_rungs(ndim)`` (16 up to ndim 128).  Not served:
    ``method="hmc"``, exchanging temperatures instead of states, adaptive ladders, the hot rungs' trajectories.

    Step-size adaptation in a warm-up, burn-in and thinning (no counterpart in the reference; ``rng="philox"``; not with
    ``temperatures``).  ``warmup=W`` (integer, ``0 <= W <= maxiter - 1``, default 0): chain c carries a multiplier
    ``s_c`` of ``stepsize`` (1.0 at the start) that samples 1 ... W adapt by dual averaging (Hoffman & Gelman 2014)
    towards the acceptance ``target_accept`` (a float in (0, 1); default 0.234, 0.44 when one variable is perturbed per
    sample; only with ``warmup > 0``); from sample W + 1 on it is frozen at its average.  The decision rule is not
    changed.  ``burn=B`` (integer, ``0 <= B <= maxiter - 1``, default ``warmup``) and ``thin=T`` (integer >= 1, default
    1): ``xall`` / ``funall`` hold samples B, B + T, B + 2T, ... ``< maxiter`` -- ``ceil((maxiter - B) / T)`` rows in
    the place of ``maxiter``.  ``x``, ``fun``, ``nit``, ``accept_ratio`` and ``accept_ratios`` stay defined over ALL
    generated samples, so ``x`` may be a sample ``xall`` does not hold.  With ``warmup > 0`` the result also has
    ``stepsizes`` (the frozen multipliers, ``(C,)``; the step in use is ``stepsizes * stepsize``),
    ``accept_ratios_sampling`` (``(C,)``: accepted samples after the warm-up over ``maxiter - 1 - W``; 0.0 when there is
    none) -- both scalars for one chain -- and ``warmup``.  The callback is called once per generated sample as before;
    its state's ``xall`` / ``funall`` hold the recorded rows among the samples before the newest.

    Per-axis scales in the warm-up (no counterpart in the reference): ``metric="diag"`` (default ``None``; needs
    ``warmup >= 20`` and ``rng="philox"``; not with ``temperatures``).  One multiplier per chain cannot serve a target whose
    axes have different widths: it settles on the narrowest.  With ``"diag"`` chain c also carries ``m_c[e]`` (1.0 at the
    start, geometric mean 1) and steps by ``s_c * m_c[e] * stepsize[e]``.  The warm-up is cut as Stan cuts it: 15 % for the
    step size alone, then up to four doubling windows (``_adapt.metric_windows``; W = 1000: ends 200, 300, 500, 900), 10 % at
    the end.  In a window the chain accumulates the variance of its own samples per axis (Welford); at a window's end
    ``m`` becomes the square root of that variance, shrunk towards ``1e-3`` of the squared half-width of the box with weight
    ``5 / (N + 5)``, over its geometric mean -- a chain whose variance is not finite or not positive on some axis keeps its
    ``m`` -- and the dual averaging restarts from its average.  Chains stay independent of each other and of ``chains``.  The
    result gains ``metric`` (``(C, ndim)``, ``(ndim,)`` for one chain: the final ``m``) and ``metric_windows`` (the ends);
    ``stepsizes`` is the final multiplier ``s_c``, so the step in use is ``stepsizes * metric * stepsize``.
    """
    if temperatures is not None or swap_every is not None:
        from . import _temper

        _adapt.refuse_with_temperatures(warmup, target_accept, burn, thin)
        _adapt.check_metric(metric, with_temperatures=True)
        ladder, every = _temper.check_ladder(temperatures, swap_every, rng)
        run = _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                            backend)
        if not 0.0 <= perc <= 1.0:
            raise ValueError()
        _temper.check_rungs(ladder, run.ndim)
        run.temperatures, run.swap_every = ladder, every
        run.method = _lib.SX_SAMPLE_MCMC
        run.k = max(1, int(perc * run.ndim))
        return _temper.run(run)
    run = _chains.Setup(fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                        backend)
    if not 0.0 <= perc <= 1.0:
        raise ValueError()
    run.method = _lib.SX_SAMPLE_MCMC
    run.k = max(1, int(perc * run.ndim))
    run.adapt = _adapt.check(warmup, target_accept, burn, thin, rng, run.maxiter, 0.44 if run.k == 1 else 0.234,
                             metric)
    return _chains.run(run)


register("mcmc", sample)
