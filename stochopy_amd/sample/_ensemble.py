"""The affine-invariant ensemble sampler (Goodman & Weare 2010, the stretch move): ensembles of device-resident walkers
(csrc/sx_sample_ensemble.hip).  No counterpart in the reference.  The checks need no device."""
import ctypes as C
import math

import numpy as np

from .. import _device, _lib
from . import _chains
from ._helpers import SampleResult, register_own

__all__ = ["sample"]

LDS_LIMIT = 160 * 1024  # what one workgroup may declare (gfx950)


def check_walkers(walkers, ndim):
    if walkers is None:
        return max(4, 2 * ndim)
    if isinstance(walkers, bool) or not isinstance(walkers, (int, np.integer)):
        raise TypeError(f"walkers (the walkers of one ensemble) is an integer, not {type(walkers).__name__}")
    if walkers < 4 or walkers % 2 or walkers < 2 * ndim:
        raise ValueError(f"walkers (the walkers of one ensemble) is even, >= 4 and >= 2 * ndim = {2 * ndim}: the two halves "
                         f"of an ensemble must span the space; got {walkers}")
    return int(walkers)


def check_stretch(stretch):
    if isinstance(stretch, bool) or not isinstance(stretch, (int, float, np.integer, np.floating)):
        raise TypeError(f"stretch (the scale a of the stretch move) is a float > 1, not {type(stretch).__name__}")
    stretch = float(stretch)
    if not math.isfinite(stretch) or stretch <= 1.0:
        raise ValueError(f"stretch (the scale a of the stretch move) is a finite float > 1, not {stretch}")
    return stretch


def largest_walkers(ndim):
    """The largest W whose ensemble of ``ndim`` variables fits one workgroup's LDS (sx_sample_ensemble_lds_bytes), or 0."""
    L = _lib.lib()

    def fits(W):
        return 0 < L.sx_sample_ensemble_lds_bytes(W, ndim) <= LDS_LIMIT

    lo = max(4, 2 * ndim)
    if not fits(lo):
        return 0
    hi = lo
    while fits(2 * hi):
        hi *= 2
    lo, hi = hi, 2 * hi  # fits(lo), not fits(hi); the bytes grow with W
    while hi - lo > 2:
        mid = (lo + hi) // 4 * 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    return lo


def check_lds(W, ndim):
    """The resident path holds an ensemble in one workgroup's LDS; around a factory.batched objective the walkers live in
    device memory and no such limit applies."""
    nbytes = int(_lib.lib().sx_sample_ensemble_lds_bytes(W, ndim))
    if 0 < nbytes <= LDS_LIMIT:
        return
    most = largest_walkers(ndim)
    fit = f"the largest walkers that fits ndim = {ndim} is {most}" if most else f"no ensemble of ndim = {ndim} variables fits (ndim <= 96 does)"
    raise ValueError(f"walkers = {W}: an ensemble of a factory objective lives in one workgroup's LDS (160 KiB; "
                     f"sx_sample_ensemble_lds_bytes), and {fit}.  A factory.batched objective has no such limit: its "
                     "walkers live in device memory")


def sample(
    fun,
    bounds,
    x0=None,
    args=(),
    maxiter=100,
    walkers=None,
    stretch=2.0,
    seed=None,
    constraints=None,
    return_all=True,
    callback=None,
    chains=1,
    rng="philox",
    backend="hip",
):
    """Sample the variable space with the affine-invariant ensemble sampler (Goodman & Weare 2010: the stretch move, the
    default move of emcee).  No counterpart in the reference.  It has no step size and needs no gradient, and it performs
    alike on ``p(x)`` and on ``p(Ax + b)`` for any invertible A: the sampler for targets whose axes are neither equally wide
    nor the coordinate axes.

    ``chains = C`` ENSEMBLES of ``walkers = W`` walkers each (W even, >= 4 and >= 2 ndim; default ``max(4, 2 ndim)``), h = W / 2.
    Sample 0 is the initial state: ``x0=None`` lets every walker draw its own point uniformly in the box; ``x0`` may be
    ``(W, ndim)`` (shared by all ensembles) or ``(C, W, ndim)``.  ``(ndim,)`` is refused: walkers that start on one point never
    move.  Sample ``it >= 1`` is two half-sweeps: the walkers ``[0, h)`` move against the walkers ``[h, W)``, then those against
    the first half as it then stands.  A walker X picks a partner X_j of the other half uniformly, draws
    ``z = ((a - 1) u + 1)^2 / a`` (``a = stretch``, default 2.0), proposes ``Y = X_j + z (X - X_j)`` and accepts with
    probability ``min(1, z^(ndim - 1) p(Y) / p(X))``, ``fun = -log p``.  With ``constraints="Reject"`` a Y outside the bounds
    is rejected (``nreject`` counts them).  Draws are made in the kernel (``rng="philox"``, an integer ``seed``), keyed by
    walker: an ensemble does not depend on ``chains``.

    ``fun`` is a ``stochopy_amd.factory`` objective -- the run is then ONE kernel launch, every ensemble in the LDS of one
    workgroup, which bounds W (``sx_sample_ensemble_lds_bytes(W, ndim) <= 160 KiB``: ndim <= 96 at W = 2 ndim) -- or a
    ``factory.batched`` device objective, called on the ``(C h, ndim)`` proposals of each half-sweep (first on the ``(C W, ndim)``
    initial points); that path has no such limit and is the resident run bit for bit for the same values.

    Result: ``x`` / ``fun`` the best ACCEPTED sample over all walkers (``fun = inf`` and ``x`` walker 0's first sample when
    nothing was accepted), ``nit = maxiter``, ``accept_ratio`` = accepted / (C W maxiter), ``accept_ratios (C, W)``,
    ``walkers``, ``stretch``, with ``return_all`` ``xall (C, maxiter, W, ndim)`` and ``funall (C, maxiter, W)`` (the leading axis
    dropped for C = 1).  The callback is called once per sample with ``xk`` the ``(C, W, ndim)`` states (squeezed likewise).

    Out of scope: ``warmup`` / ``burn`` / ``thin``, other moves (differential evolution, walk), tempering,
    ``rng="numpy-legacy"``, and ensembles larger than one workgroup's LDS on the resident path.
    """
    # the reference-style refusals, in _chains.Setup's order
    if not hasattr(fun, "__call__"):
        raise TypeError()
    if np.ndim(bounds) != 2:
        raise ValueError()
    if callback is not None and not hasattr(callback, "__call__"):
        raise ValueError()
    ndim = len(bounds)
    if isinstance(chains, bool) or int(chains) != chains or chains < 1:
        raise ValueError("chains is an integer >= 1")
    chains = int(chains)
    W = check_walkers(walkers, ndim)
    a = check_stretch(stretch)
    if rng != "philox":
        raise ValueError(f'rng={rng!r}: method="ensemble" makes its draws in the kernel, keyed by walker: rng="philox"')
    if seed is None or isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError('seed: method="ensemble" (rng="philox") needs an explicit integer seed')
    if x0 is not None:
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.shape == (W, ndim):
            x0 = np.tile(x0, (chains, 1))
        elif x0.shape == (chains, W, ndim):
            x0 = x0.reshape(chains * W, ndim)
        else:
            raise ValueError(f"x0 is (walkers, ndim) = {(W, ndim)}, shared by all ensembles, or (chains, walkers, ndim) = "
                             f"{(chains, W, ndim)}, not {x0.shape}: walkers that start on one point never move")
        x0 = np.ascontiguousarray(x0)
    # the rest of the conditions every sampler shares (fun, ndim, maxiter, constraints, backend)
    s = _chains.Setup(fun, bounds, None, args, maxiter, 0.1, seed, constraints, return_all, callback, chains, rng, backend)
    s.method = _lib.SX_SAMPLE_ENSEMBLE
    s.x0, s.walkers, s.stretch = x0, W, a
    if s.external is None:
        check_lds(W, ndim)
    return run(s)


def run(s):
    L = _lib.lib()
    Cn, W, n, m = s.chains, s.walkers, s.ndim, s.maxiter
    h, R = W // 2, Cn * W  # replicas: q = g * W + w is walker w of ensemble g
    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        on_device_all = s.return_all and s.callback is None
        dev, a = _chains.chain_args(ctx, s, None, chains=R, x0=s.x0)
        if on_device_all:
            dev["xall"] = ctx.empty((Cn, m, W, n))
            dev["funall"] = ctx.empty((Cn, m, W))
            a.xall, a.funall = _device.ptr(dev["xall"]), _device.ptr(dev["funall"])
        ptr = _device.ptr

        def host(name):
            return dev[name].cpu().numpy()

        if s.external is not None:
            prop = ctx.empty((R, n))
            logzf = ctx.empty((Cn * h,))

            def half_sweep(it, half, P):
                _lib.check(L.sx_sample_ensemble_propose(C.byref(a), W, s.stretch, it, half, ptr(P), ptr(logzf), ctx.stream_ptr),
                           "sx_sample_ensemble_propose")
                f = s.external(ctx, P)
                _lib.check(L.sx_sample_ensemble_decide(C.byref(a), W, it, half, ptr(P), ptr(f), ptr(logzf), ctx.stream_ptr),
                           "sx_sample_ensemble_decide")

            def advance(i, steps):
                for it in range(i, i + steps):
                    if it == 0:
                        half_sweep(0, 0, prop)
                    else:
                        half_sweep(it, 0, prop[:Cn * h])
                        half_sweep(it, 1, prop[:Cn * h])
        else:
            def advance(i, steps):  # one launch
                _lib.check(L.sx_sample_ensemble_run(C.byref(a), W, s.stretch, i, steps, ctx.stream_ptr), "sx_sample_ensemble_run")

        def squeeze(v):
            return v[0] if Cn == 1 else v

        if s.callback is None:
            advance(0, m)
            xall = host("xall") if on_device_all else None
            funall = host("funall") if on_device_all else None
        else:
            # one launch per sample; the state the callback sees is assembled as mcmc's: x / fun = the best ACCEPTED sample so
            # far (walker 0's first sample while there is none), xall / funall WITHOUT the newest
            xall = np.empty((Cn, m, W, n))
            funall = np.empty((Cn, m, W))
            for i in range(m):
                advance(i, 1)
                xall[:, i] = host("cur").reshape(Cn, W, n)
                funall[:, i] = host("fcur").reshape(Cn, W)
                iacc = host("iacc")
                facc_now = np.where(iacc == 0, funall[:, 0].reshape(R), host("facc"))
                b = int(np.argmin(facc_now))
                state = SampleResult(x=host("xbest")[b], fun=facc_now[b], nit=i + 1,
                                     accept_ratio=1.0 if i == 0 else int(host("nacc").sum()) / (R * (i + 1)))
                if s.return_all:
                    upto = max(i, 1)
                    state.update({"xall": squeeze(xall[:, :upto]), "funall": squeeze(funall[:, :upto])})
                s.callback(squeeze(xall[:, i]), state)
        ctx.sync()
        nacc, nfeas = host("nacc"), host("nfeas")
        fbest, xbest = host("facc"), host("xbest")
    b = int(np.argmin(fbest))  # (numpy's rule; all inf: walker 0 of ensemble 0, whose xbest is its first sample)
    res = SampleResult(x=xbest[b], fun=fbest[b], nit=m, accept_ratio=int(nacc.sum()) / (R * m))
    if s.reject:
        res["nreject"] = R * (m - 1) - int(nfeas.sum())  # proposals that left the box
    res["accept_ratios"] = nacc.reshape(Cn, W) / m
    res["walkers"], res["stretch"] = W, s.stretch
    if s.return_all:
        res["xall"], res["funall"] = squeeze(xall), squeeze(funall)
    return res


register_own("ensemble", sample)
