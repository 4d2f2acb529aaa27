"""Tempered sequential Monte Carlo with the evidence (Del Moral et al. 2006; TMCMC, Ching & Chen 2007): populations of
device-resident particles walked from the uniform prior on the box to the target (csrc/sx_sample_smc.hip).  No counterpart in
the reference.  The checks need no device."""
import ctypes as C
import math

import numpy as np

from .. import _device, _lib
from . import _chains
from ._helpers import SampleResult, register_own

__all__ = ["sample"]

RUNNING = 1  # (the record's status while a population goes on; sx_sample_smc.hip)
ST_STATUS, ST_BETA, ST_LOGZ, ST_ESS, ST_SCALE, ST_ACCEPT, ST_STAGES, ST_COUNT, ST_WORDS = range(9)


def _integer(value):
    return not isinstance(value, bool) and isinstance(value, (int, np.integer))


def _number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))


def max_particles():
    """The most particles of one population: their values live in one workgroup's LDS (sx_smc_max_particles)."""
    return int(_lib.lib().sx_smc_max_particles())


def check_particles(particles):
    if not _integer(particles):
        raise TypeError(f"particles (the particles of one population) is an integer, not {type(particles).__name__}")
    if not 4 <= particles <= max_particles():
        raise ValueError(f"particles (the particles of one population) is 4 ... {max_particles()}: the values of a population "
                         f"live in one workgroup's LDS; got {particles}")
    return int(particles)


def check_steps(steps):
    if not _integer(steps):
        raise TypeError(f"steps (the Metropolis steps of a particle per stage) is an integer, not {type(steps).__name__}")
    if steps < 1:
        raise ValueError(f"steps (the Metropolis steps of a particle per stage) is >= 1, not {steps}")
    return int(steps)


def check_fraction(name, what, value):
    if not _number(value):
        raise TypeError(f"{name} ({what}) is a float in (0, 1), not {type(value).__name__}")
    value = float(value)
    if not 0.0 < value < 1.0:  # (a NaN fails both)
        raise ValueError(f"{name} ({what}) is a float in (0, 1), not {value}")
    return value


def check_scale(scale, ndim):
    if scale is None:
        return 2.38 / math.sqrt(ndim)
    if not _number(scale):
        raise TypeError(f"scale (the first stage's proposal scale) is None or a finite float > 0, not {type(scale).__name__}")
    scale = float(scale)
    if not math.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"scale (the first stage's proposal scale) is None or a finite float > 0, not {scale}")
    return scale


def sample(
    fun,
    bounds,
    x0=None,
    args=(),
    maxiter=100,
    particles=1024,
    chains=1,
    steps=8,
    ess=0.5,
    target_accept=0.234,
    scale=None,
    seed=None,
    callback=None,
    rng="philox",
    backend="hip",
):
    """Sample ``exp(-fun)`` on the box AND estimate its evidence with a tempered sequential Monte Carlo sampler (Del Moral
    et al. 2006; TMCMC, Ching & Chen 2007; the rule of PyMC's ``sample_smc``).  No counterpart in the reference.  ``fun`` is
    minus the log likelihood, the prior is uniform on ``bounds``, and ``log_evidence`` is the log of
    ``Z = integral of exp(-fun(x)) dx / volume of the box``, the marginal likelihood -- what chains and ensembles cannot give.
    The sampler chooses its own ladder of inverse temperatures, and finds the weights of separated modes from a cold start.

    ``chains = C`` POPULATIONS of ``particles = P`` particles (4 ... 16 384, default 1 024), independent of each other and of
    C.  Stage 0 draws every particle uniformly in the box (``x0`` is refused) at ``beta = 0``.  Stage s then

    1. picks the next beta: 1 when the effective sample size of the weights ``exp(-(beta - beta_prev)(f - min f))`` at
       beta = 1 is at least ``ess * P`` (default 0.5), else by 52 halvings of ``[beta_prev, 1]`` the largest beta that keeps it;
    2. adds ``log(mean weight)`` to the log evidence;
    3. resamples the particles systematically by their weights;
    4. sets the step of every axis to ``scale_s`` times the population's standard deviation on it (``scale_1 = scale``,
       default ``2.38 / sqrt(ndim)``; never below 1e-8 of the half-width: a collapsed population keeps moving);
    5. moves every particle by ``steps = M`` Metropolis steps (default 8) on ``exp(-beta fun)``, every variable at once, a
       proposal outside the box rejected;
    6. ``scale_{s+1} = scale_s exp(r_s - target_accept)``, r_s the share of accepted steps (default target 0.234).

    A population ends after the moves of the stage with beta = 1 (status 0), after ``maxiter`` stages with beta < 1 (status -1:
    its particles sample ``p^beta``), or where no particle has a finite value or one has -inf (status -2, evidence -inf); the
    others go on.  Draws are made in the kernels (``rng="philox"``, an integer ``seed``), keyed by particle.

    ``fun`` is a ``stochopy_amd.factory`` objective -- a stage is then three launches, the moves resident in LDS -- or a
    ``factory.batched`` device objective, called on the ``(C P, ndim)`` particles first and on their proposals at every step;
    for the same values that is the resident run bit for bit.  The host reads C small records per stage, nothing else.

    Result: ``xall (C, P, ndim)`` / ``funall (C, P)`` the final, equally weighted particles (the leading axis dropped for
    C = 1, here and below), ``x`` / ``fun`` numpy's argmin over ``funall``, ``log_evidence (C,)``, ``betas (C, S + 1)`` (S the
    stages of the longest population, rows padded with their last value), ``stages (C,)``, ``statuses (C,)``, ``status`` the
    worst of them, ``accept_ratios`` / ``scales`` / ``ess`` ``(C, S)`` (0 where a population had ended), ``accept_ratio``
    accepted over attempted steps, ``nit = S``, ``nfev = sum_c P (1 + M stages_c)``, ``particles``.  A callback is called after
    every stage with ``(xk (C, P, ndim), state)``, ``state`` holding ``nit``, ``betas`` and ``log_evidence`` so far.

    Out of scope: HMC or independent / full-covariance proposals in the moves, ``x0``, an adaptive ``steps``, weighted output
    without the final resampling, more particles per population than one workgroup's LDS holds, rows wider than the
    wavefront-per-row kernels serve, ``rng="numpy-legacy"``, several GPUs.
    """
    # the reference-style refusals, in _chains.Setup's order
    if not hasattr(fun, "__call__"):
        raise TypeError()
    if np.ndim(bounds) != 2:
        raise ValueError()
    if callback is not None and not hasattr(callback, "__call__"):
        raise ValueError()
    if x0 is not None:
        raise ValueError('x0: method="smc" draws its particles from the prior, uniformly in the box; x0 must be None')
    ndim = len(bounds)
    if isinstance(chains, bool) or int(chains) != chains or chains < 1:
        raise ValueError("chains is an integer >= 1")
    P = check_particles(particles)
    M = check_steps(steps)
    ess = check_fraction("ess", "the share of the particles the effective sample size is kept at", ess)
    target = check_fraction("target_accept", "the acceptance ratio the scale is steered to", target_accept)
    scale = check_scale(scale, ndim)
    if rng != "philox":
        raise ValueError(f'rng={rng!r}: method="smc" makes its draws in the kernels, keyed by particle: rng="philox"')
    if seed is None or isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError('seed: method="smc" (rng="philox") needs an explicit integer seed')
    # the rest of the conditions every sampler shares (fun, args, ndim, maxiter, backend)
    s = _chains.Setup(fun, bounds, None, args, maxiter, 0.1, seed, None, True, callback, chains, rng, backend)
    if s.maxiter * M >= 1 << 31:
        raise ValueError(f"maxiter * steps = {s.maxiter * M}: the steps of a particle are numbered below 2^31")
    if s.chains * P >= 1 << 31:
        raise ValueError(f"chains * particles = {s.chains * P}: the particles are numbered below 2^31")
    s.particles, s.steps, s.ess, s.target, s.scale = P, M, ess, target, scale
    return run(s)


def smc_args(ctx, s):
    """``(dev, a)``: the device arrays of a run of ``s`` and the SxSmcArgs that points at them, on the current stream."""
    t = _device.torch()
    Cn, P, n = s.chains, s.particles, s.ndim
    R = Cn * P
    dev = {"x0": ctx.zeros((R, n)), "x1": ctx.zeros((R, n)), "f0": ctx.zeros((R,)), "f1": ctx.zeros((R,)),
           "anc": ctx.zeros((R,), dtype=t.int32), "nacc": ctx.zeros((R,), dtype=t.int64), "step": ctx.zeros((Cn, n)),
           "state": ctx.zeros((Cn, ST_WORDS)), "lower": ctx.upload(s.lower), "upper": ctx.upload(s.upper)}
    a = _lib.SxSmcArgs()
    ptr = _device.ptr
    a.x[0], a.x[1], a.f[0], a.f[1] = (ptr(dev[k]).value for k in ("x0", "x1", "f0", "f1"))
    for name in ("anc", "nacc", "step", "state", "lower", "upper"):
        setattr(a, name, ptr(dev[name]))
    a.C, a.P, a.n, a.fun_id, a.steps, a.maxiter = Cn, P, n, s.fun_id, s.steps, s.maxiter
    a.ess, a.target, a.scale = s.ess, s.target, s.scale
    a.key0, a.key1 = s.key
    return dev, a


def run(s):
    L = _lib.lib()
    Cn, P, n, M = s.chains, s.particles, s.ndim, s.steps
    ctx = _device.Context()
    t = _device.torch()
    ptr = _device.ptr
    betas, logzs, esss, scales, ratios, counts = [np.zeros(Cn)], [np.zeros(Cn)], [], [], [], []
    with t.cuda.stream(ctx.stream):
        dev, a = smc_args(ctx, s)

        def call(name, *args):
            _lib.check(getattr(L, name)(C.byref(a), *args, ctx.stream_ptr), name)

        def records():  # the one read of a stage
            return dev["state"].cpu().numpy()

        if s.external is None:
            call("sx_smc_init")

            def mutate(stage):
                call("sx_smc_mutate", stage)
        else:
            prop = ctx.zeros((Cn * P, n))
            call("sx_smc_propose", 0, 0, ptr(prop))
            call("sx_smc_decide", 0, 0, ptr(prop), ptr(s.external(ctx, prop)))

            def mutate(stage):
                for m in range(1, M + 1):
                    call("sx_smc_propose", stage, m, ptr(prop))
                    call("sx_smc_decide", stage, m, ptr(prop), ptr(s.external(ctx, prop)))

        def particles(stages):
            """(C, P, n), (C, P): every population from the buffer its last stage worked in."""
            odd = t.from_numpy((stages % 2).astype(bool)).to(dev["x0"].device)
            x = t.where(odd.repeat_interleave(P)[:, None], dev["x1"], dev["x0"])
            f = t.where(odd.repeat_interleave(P), dev["f1"], dev["f0"])
            return x.cpu().numpy().reshape(Cn, P, n), f.cpu().numpy().reshape(Cn, P)

        stages = np.zeros(Cn, dtype=np.int64)
        status = np.full(Cn, RUNNING, dtype=np.int64)
        S, closed = 0, False
        while np.any(status == RUNNING):  # (maxiter stages end every population: status -1)
            S += 1
            call("sx_smc_stage", S)
            call("sx_smc_resample", S)
            mutate(S)
            rec = records()
            before, stages = stages, rec[:, ST_STAGES].astype(np.int64)
            status = rec[:, ST_STATUS].astype(np.int64)
            took = stages == S  # the populations that took part in this stage
            if S >= 2:  # step 6 of the stage before, for those that took part in it
                ratios.append(np.where(before == S - 1, rec[:, ST_ACCEPT], 0.0))
                counts.append(np.where(before == S - 1, rec[:, ST_COUNT], 0.0))
            if not np.any(took):  # (every population still running ended at the start of this stage: status -2)
                S, closed = S - 1, True
                logzs.append(rec[:, ST_LOGZ])
                break
            betas.append(rec[:, ST_BETA])
            logzs.append(rec[:, ST_LOGZ])
            esss.append(np.where(took, rec[:, ST_ESS], 0.0))
            scales.append(np.where(took, rec[:, ST_SCALE], 0.0))
            if s.callback is not None:
                xk = particles(stages)[0]
                state = SampleResult(nit=S, betas=_squeeze(np.array(betas).T, Cn), log_evidence=_squeeze(rec[:, ST_LOGZ].copy(), Cn))
                s.callback(_squeeze(xk, Cn), state)
        if S >= 1 and not closed:  # step 6 of the last stage
            call("sx_smc_stage", S + 1)
            rec = records()
            ratios.append(np.where(stages == S, rec[:, ST_ACCEPT], 0.0))
            counts.append(np.where(stages == S, rec[:, ST_COUNT], 0.0))
        xall, funall = particles(stages)
        ctx.sync()
    b = int(np.argmin(funall))  # (numpy's rule: the first NaN, else the first minimum)
    res = SampleResult(x=xall.reshape(Cn * P, n)[b], fun=funall.reshape(Cn * P)[b], nit=S)
    attempted = P * M * int(stages.sum())
    res["accept_ratio"] = float(np.sum(counts)) / attempted if attempted else 0.0
    res["nfev"] = int(np.sum(P * (1 + M * stages)))
    res["status"] = int(status.min())
    res["particles"] = P
    for name, value in (("xall", xall), ("funall", funall), ("log_evidence", logzs[-1].copy()),
                        ("betas", np.array(betas).T), ("stages", stages), ("statuses", status),
                        ("accept_ratios", np.array(ratios).reshape(S, Cn).T), ("scales", np.array(scales).reshape(S, Cn).T),
                        ("ess", np.array(esss).reshape(S, Cn).T)):
        res[name] = _squeeze(np.ascontiguousarray(value), Cn)
    return res


def _squeeze(v, Cn):
    return v[0] if Cn == 1 else v


register_own("smc", sample)
