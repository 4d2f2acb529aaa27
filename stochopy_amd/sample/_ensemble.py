"""The affine-invariant ensemble sampler (Goodman & Weare 2010, the stretch move): ensembles of device-resident walkers
(csrc/sx_sample_ensemble.hip), and its other moves -- differential evolution, snooker -- with a burn-in and thinning
(csrc/sx_sample_ensemble_moves.hip).  No counterpart in the reference.  The checks need no device."""
import ctypes as C
import math

import numpy as np

from .. import _device, _lib
from . import _adapt, _chains
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


MOVE_KINDS = {"stretch": _lib.SX_ENSEMBLE_STRETCH, "de": _lib.SX_ENSEMBLE_DE, "snooker": _lib.SX_ENSEMBLE_SNOOKER}
MAX_MOVES = 4  # (sx_sample_ensemble_opts)


def _number(value):
    return not isinstance(value, bool) and isinstance(value, (int, float, np.integer, np.floating))


def check_moves(moves, ndim, W, stretch):
    """``([(name, weight, param)], cum)``: the checked entries with normalised weights and parameters filled in, and the running
    sums of the weights as the kernels read them (the last one 1.0)."""
    rule = ('moves (the moves of an ensemble) is a name or a sequence of 1 to 4 entries name, (name, weight) or '
            '(name, weight, param), name one of "stretch", "de", "snooker"')
    if isinstance(moves, str):
        moves = [moves]
    elif not isinstance(moves, (list, tuple)):
        raise TypeError(f"{rule}, not {type(moves).__name__}")
    if not 1 <= len(moves) <= MAX_MOVES:
        raise ValueError(f"{rule}; got {len(moves)} entries")
    entries = []
    for entry in moves:
        if isinstance(entry, str):
            entry = (entry,)
        if not isinstance(entry, (list, tuple)) or not 1 <= len(entry) <= 3 or not isinstance(entry[0], str):
            raise TypeError(f"{rule}; got the entry {entry!r}")
        name = entry[0]
        if name not in MOVE_KINDS:
            raise ValueError(f"{rule}; got the name {name!r}")
        weight = entry[1] if len(entry) > 1 else 1.0
        if not _number(weight):
            raise TypeError(f"moves: the weight of {name!r} is a finite float > 0, not {type(weight).__name__}")
        weight = float(weight)
        if not math.isfinite(weight) or weight <= 0.0:
            raise ValueError(f"moves: the weight of {name!r} is a finite float > 0, not {weight}")
        param = entry[2] if len(entry) > 2 else None
        what = {"stretch": "the scale a of the stretch move, a finite float > 1",
                "de": "gamma0 of the differential-evolution move, a finite float > 0",
                "snooker": "gamma_s of the snooker move, a finite float > 0"}[name]
        if param is None:
            param = {"stretch": stretch, "de": 2.38 / math.sqrt(2.0 * ndim), "snooker": 1.7}[name]
        elif not _number(param):
            raise TypeError(f"moves: the param of {name!r} is {what}, not {type(param).__name__}")
        param = float(param)
        if not math.isfinite(param) or param <= (1.0 if name == "stretch" else 0.0):
            raise ValueError(f"moves: the param of {name!r} is {what}, not {param}")
        if name == "snooker" and W < 6:
            raise ValueError(f'moves: "snooker" draws three distinct walkers from a half of the ensemble: it needs walkers >= 6, '
                             f"not {W}")
        entries.append((name, weight, param))
    w = np.array([e[1] for e in entries], dtype=np.float64)
    p = w / w.sum()
    cum = np.cumsum(p)
    cum[-1] = 1.0
    if not np.all(np.isfinite(p)) or not np.all(np.diff(np.concatenate(([0.0], cum))) > 0.0):
        raise ValueError("moves: the weights are so unequal that their normalised running sums do not increase")
    return [(e[0], float(pk), e[2]) for e, pk in zip(entries, p)], cum


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
    moves=None,
    burn=0,
    thin=1,
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

    ``moves``: the stretch proposal lies on the line through two walkers, at 1/a to a times their distance from the partner:
    it cannot carry a walker from one mode of a target into another, and an ensemble keeps the split between separated modes
    that its starting points gave it.  ``moves`` is a name or a sequence of 1 to 4 entries ``name``, ``(name, weight)`` or
    ``(name, weight, param)``; per sample each ensemble picks one entry with probability weight / sum of the weights (finite,
    > 0, default 1) and uses it in both half-sweeps.  A name may occur more than once.

    - ``"stretch"``: the move above, ``param`` its scale a > 1 (default ``stretch``).
    - ``"de"`` (ter Braak 2006): ``Y = X + g (X_j1 - X_j2)`` with two distinct walkers of the other half and
      ``g = param (1 + 1e-5 (2 u - 1))``; ``param`` > 0, default ``2.38 / sqrt(2 ndim)``.  Accepted with ``min(1, p(Y) / p(X))``.
    - ``"snooker"`` (ter Braak & Vrugt 2008): with three distinct walkers Z, Z1, Z2 of the other half (``walkers >= 6``),
      ``Y = X + c (X - Z)``, c = ``param`` times the projection of Z1 - Z2 on X - Z over |X - Z|^2; ``param`` > 0, default 1.7.
      Accepted with ``min(1, |1 + c|^(ndim - 1) p(Y) / p(X))``.

    ``[("de", 0.7), ("de", 0.1, 1.0), ("snooker", 0.2)]`` is the mixture to use on targets with separated modes.
    ``moves=None`` is the stretch move alone.

    ``burn=B`` (integer, ``0 <= B <= maxiter - 1``, default 0) and ``thin=T`` (integer >= 1, default 1): ``xall`` / ``funall``
    hold samples ``B, B + T, ...`` only, ``ceil((maxiter - B) / T)`` rows in the place of ``maxiter``; the counts,
    ``accept_ratio`` / ``accept_ratios`` and ``x`` / ``fun`` still run over all samples, and a callback is still called once
    per sample, its ``state.xall`` / ``funall`` holding the recorded rows among the samples before the newest.  When any of
    the three is given the result carries ``moves`` (the checked entries ``(name, weight, param)`` with normalised weights),
    ``burn`` and ``thin``.

    Out of scope: ``warmup``, per-move acceptance counts, the walk move, tempering, ``rng="numpy-legacy"``, several GPUs, and
    ensembles larger than one workgroup's LDS on the resident path.
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
    checked = None if moves is None else check_moves(moves, ndim, W, a)
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
    # burn / thin: the ranges and messages of mcmc's (None when both are at their defaults)
    s.adapt = _adapt.check(0, None, None if _adapt._is(burn, 0) else burn, thin, rng, s.maxiter, 0.5)
    s.moves = None
    if checked is not None or s.adapt is not None:
        s.moves, s.cum = checked if checked is not None else check_moves("stretch", ndim, W, a)
        if s.adapt is None:
            s.adapt = _adapt.Adapt(0, 0.5, 0, 1, s.maxiter)
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
        rows = m if s.moves is None else s.adapt.rows  # (burn / thin: the rows of xall / funall per ensemble)
        if on_device_all:
            dev["xall"] = ctx.empty((Cn, rows, W, n))
            dev["funall"] = ctx.empty((Cn, rows, W))
            a.xall, a.funall = _device.ptr(dev["xall"]), _device.ptr(dev["funall"])
        ptr = _device.ptr
        mv = None
        if s.moves is not None:  # moves / burn / thin: the *_moves entry points, the options in their own struct
            mv = _lib.SxSampleEnsembleOpts()
            mv.nmoves = len(s.moves)
            for k, (name, _, param) in enumerate(s.moves):
                mv.kind[k], mv.cum[k], mv.param[k] = MOVE_KINDS[name], s.cum[k], param
            mv.rec_start, mv.rec_rows = s.adapt.burn, rows
            mv.rec_every = min(s.adapt.thin, m)  # (the same rows; the library takes rec_every < 2^31)

        def host(name):
            return dev[name].cpu().numpy()

        if s.external is not None:
            prop = ctx.empty((R, n))
            logzf = ctx.empty((Cn * h,))

            def half_sweep(it, half, P):
                if mv is None:
                    _lib.check(L.sx_sample_ensemble_propose(C.byref(a), W, s.stretch, it, half, ptr(P), ptr(logzf), ctx.stream_ptr),
                               "sx_sample_ensemble_propose")
                else:
                    _lib.check(L.sx_sample_ensemble_propose_moves(C.byref(a), W, C.byref(mv), it, half, ptr(P), ptr(logzf),
                                                                  ctx.stream_ptr), "sx_sample_ensemble_propose_moves")
                f = s.external(ctx, P)
                if mv is None:
                    _lib.check(L.sx_sample_ensemble_decide(C.byref(a), W, it, half, ptr(P), ptr(f), ptr(logzf), ctx.stream_ptr),
                               "sx_sample_ensemble_decide")
                else:
                    _lib.check(L.sx_sample_ensemble_decide_moves(C.byref(a), W, C.byref(mv), it, half, ptr(P), ptr(f), ptr(logzf),
                                                                 ctx.stream_ptr), "sx_sample_ensemble_decide_moves")

            def advance(i, steps):
                for it in range(i, i + steps):
                    if it == 0:
                        half_sweep(0, 0, prop)
                    else:
                        half_sweep(it, 0, prop[:Cn * h])
                        half_sweep(it, 1, prop[:Cn * h])
        else:
            def advance(i, steps):  # one launch
                if mv is None:
                    _lib.check(L.sx_sample_ensemble_run(C.byref(a), W, s.stretch, i, steps, ctx.stream_ptr), "sx_sample_ensemble_run")
                else:
                    _lib.check(L.sx_sample_ensemble_run_moves(C.byref(a), W, C.byref(mv), i, steps, ctx.stream_ptr),
                               "sx_sample_ensemble_run_moves")

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
                    if mv is not None:  # the recorded rows among the samples before the newest (as mcmc's burn / thin)
                        upto = s.adapt.recorded[s.adapt.recorded < upto]
                    else:
                        upto = slice(0, upto)
                    state.update({"xall": squeeze(xall[:, upto]), "funall": squeeze(funall[:, upto])})
                s.callback(squeeze(xall[:, i]), state)
            if mv is not None:
                xall, funall = xall[:, s.adapt.recorded], funall[:, s.adapt.recorded]
        ctx.sync()
        nacc, nfeas = host("nacc"), host("nfeas")
        fbest, xbest = host("facc"), host("xbest")
    b = int(np.argmin(fbest))  # (numpy's rule; all inf: walker 0 of ensemble 0, whose xbest is its first sample)
    res = SampleResult(x=xbest[b], fun=fbest[b], nit=m, accept_ratio=int(nacc.sum()) / (R * m))
    if s.reject:
        res["nreject"] = R * (m - 1) - int(nfeas.sum())  # proposals that left the box
    res["accept_ratios"] = nacc.reshape(Cn, W) / m
    res["walkers"], res["stretch"] = W, s.stretch
    if s.moves is not None:
        res["moves"], res["burn"], res["thin"] = list(s.moves), s.adapt.burn, s.adapt.thin
    if s.return_all:
        res["xall"], res["funall"] = squeeze(xall), squeeze(funall)
    return res


register_own("ensemble", sample)
