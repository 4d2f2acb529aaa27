"""What both samplers share: argument checks (no device needed), the draws of the numpy-legacy mode, the launches of the
chain kernels (csrc/sx_sample.hip; around a caller's own objective: csrc/sx_sample_unfused.hip) and the assembly of the
result."""
import ctypes as C

import numpy as np

from .. import _device, _lib, _rng
from ..factory.benchmark import Objective, batched
from ..optimize._common import External
from ._helpers import SampleResult

# hmc with a factory.batched objective and jac=None: the finite differences' rows of one chunk of axes are stacked into one
# (axes, 2, chains, ndim) array so that ONE call of the caller's objective evaluates them; the chunk is as many axes as keep
# that array under this many bytes (at least one)
FD_STACK_BYTES = 256 << 20


def fd_axes_per_chunk(chains, ndim):
    """Axes whose 2 * chains finite-difference rows of ndim doubles fit FD_STACK_BYTES: 1 ... ndim."""
    return max(1, min(ndim, FD_STACK_BYTES // (2 * chains * ndim * 8)))


class Gradient:
    """A caller-supplied gradient (``jac=factory.batched(g)``) as the hmc loop uses it: ``grad(ctx, X)`` -> (C, n) device
    tensor.  Checked as ``optimize._common.External`` checks an objective."""

    def __init__(self, tagged, args):
        self.fun = tagged.fun
        self.args = tuple(args) if args not in ((), None) else ()
        self.name = tagged.__name__

    def __call__(self, ctx, X):
        t = _device.torch()
        g = self.fun(X, *self.args)
        if not isinstance(g, t.Tensor) or g.device != X.device:
            raise TypeError(f"batched gradient {self.name}: expected a tensor on {X.device}, got {type(g).__name__}")
        if g.shape != X.shape:
            raise ValueError(f"batched gradient {self.name}: expected shape {tuple(X.shape)}, got {tuple(g.shape)}")
        return g.to(t.float64).contiguous()


class AutogradGradient:
    """``jac="autograd"``: the chains' rows are independent, so the gradient of ``fun(X).sum()`` with respect to X holds
    every chain's own gradient in its row."""

    def __init__(self, external):
        self.external = external

    def __call__(self, ctx, X):
        t = _device.torch()
        with t.enable_grad():
            Xg = X.detach().requires_grad_(True)
            (g,) = t.autograd.grad(self.external(ctx, Xg).sum(), Xg)
        return g.to(t.float64).contiguous()


class Setup:
    """The checked arguments of one run.  Raises what the reference raises, in its order (mcmc/_mcmc.py:62-88,
    hmc/_hmc.py:83-121), then this backend's own errors -- all before the device is touched."""

    k = 1
    nleap = 1
    jac = _lib.SX_JAC_FINITE_DIFF
    fd_step = 1.0e-4
    external = None  # a factory.batched objective: optimize._common.External (the chain kernels then run unfused)
    gradient = None  # hmc with such an objective: Gradient / AutogradGradient, or None for finite differences

    temperatures = None  # parallel tempering (mcmc, _temper.py): the ladder as float64 (K,), and
    swap_every = None    # the samples between two exchange events

    adapt = None  # warmup / target_accept / burn / thin (_adapt.py): the checked _adapt.Adapt, or None for the plain path

    def __init__(self, fun, bounds, x0, args, maxiter, stepsize, seed, constraints, return_all, callback, chains, rng,
                 backend, nleap=None):
        if not hasattr(fun, "__call__"):
            raise TypeError()
        if np.ndim(bounds) != 2:
            raise ValueError()
        self.ndim = ndim = len(bounds)
        lower, upper = np.transpose(bounds)
        self.lower = np.ascontiguousarray(lower, dtype=np.float64)
        self.upper = np.ascontiguousarray(upper, dtype=np.float64)
        if isinstance(chains, bool) or int(chains) != chains or chains < 1:
            raise ValueError("chains is an integer >= 1")
        self.chains = chains = int(chains)
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64)
            if not (x0.shape == (ndim,) or (chains > 1 and x0.shape == (chains, ndim))):
                raise ValueError()
            x0 = np.ascontiguousarray(x0)
        self.x0 = x0
        if nleap is not None and nleap < 1:
            raise ValueError()
        if np.ndim(stepsize) == 0:
            stepsize = np.full(ndim, stepsize, dtype=np.float64)
        if len(stepsize) != ndim:
            raise ValueError()
        self.step = np.array(stepsize, dtype=np.float64) * (0.5 * (self.upper - self.lower))
        if callback is not None and not hasattr(callback, "__call__"):
            raise ValueError()
        self.callback = callback
        # -- this backend's own conditions
        if backend != "hip":
            raise ValueError(f'unknown backend {backend!r}: "hip" is the only one')
        if isinstance(fun, batched):
            if rng == "numpy-legacy":
                raise TypeError('a factory.batched objective needs rng="philox": rng="numpy-legacy" replays the one stream '
                                "of the reference inside the fused chain kernels")
            self.external = External(fun, args)
            self.fun_id = 0  # (not read by the unfused kernels)
        elif not isinstance(fun, Objective):
            raise TypeError("stochopy_amd.sample runs the chains on the device: fun must be one of the stochopy_amd.factory "
                            "objectives or a device objective tagged with factory.batched (plain Python callables are not "
                            "supported)")
        else:
            if args not in ((), None):
                raise TypeError("factory objectives take no extra args")
            self.fun_id = fun.sx_id
        # (csrc/sx_device.hpp kWideFrom: the longest row the kernels with one row per wavefront take)
        if ndim < 1 or ndim > _lib.wide_from():
            raise ValueError(f"stochopy_amd.sample serves rows of 1 to {_lib.wide_from()} elements, not {ndim}")
        if isinstance(maxiter, bool) or int(maxiter) != maxiter or maxiter < 1:
            raise ValueError("maxiter is an integer >= 1")
        self.maxiter = int(maxiter)
        if constraints not in (None, "Reject"):
            raise ValueError(f"unknown constraints {constraints!r}: None or 'Reject'")
        self.reject = constraints == "Reject"
        if rng not in ("numpy-legacy", "philox"):
            raise ValueError(f'unknown rng {rng!r}: "numpy-legacy" or "philox"')
        self.rng = rng
        if rng == "numpy-legacy":
            if chains != 1:
                raise ValueError('rng="numpy-legacy" replays the one stream of the reference and serves one chain; '
                                 'use rng="philox" for chains > 1')
            if self.reject:
                raise ValueError('with constraints="Reject" the draw sequence depends on the data; use rng="philox"')
            self.key = (0, 0)
        else:
            self.key = _rng.philox_key(seed)
        self.seed = seed
        self.return_all = bool(return_all)


def _legacy_draws(s):
    """The whole run's draws from the reference's stream, in its order: the initial point when none is given, then per
    sample the normals (mcmc: the block's, hmc: ndim momenta) and the acceptance uniform.  With constraints=None the
    sequence does not depend on the data."""
    stream = _rng.LegacyHostStream(s.seed)
    n, m = s.ndim, s.maxiter
    x0 = s.x0 if s.x0 is not None else stream.uniform_rows(s.lower, s.upper, 1)[0]
    width = s.k if s.method == _lib.SX_SAMPLE_MCMC else n
    normals = np.zeros((max(m - 1, 1), width))
    u = np.ones(m)
    nblocks = -(-n // s.k)
    for i in range(1, m):
        if s.method == _lib.SX_SAMPLE_MCMC:
            j0 = ((i - 1) % nblocks) * s.k
            kb = min(s.k, n - j0)
        else:
            kb = n
        stream.randn(kb, out=normals[i - 1, :kb])
        stream.random(1, out=u[i:i + 1])
    with np.errstate(divide="ignore"):
        logu = np.log(u)
    return stream, np.ascontiguousarray(x0, dtype=np.float64), normals, logu


class _Unfused:
    """One sample around a caller-supplied objective (csrc/sx_sample_unfused.hip), launched eagerly on the engine's stream:
    propose -> fun -> decide; hmc puts nleap + 2 rounds of (gradient, leap) in front of fun.  The chains' state stays in the
    arrays of ``a``, as between the launches of a fused run with a callback."""

    def __init__(self, s, ctx, a, ad=None, mt=None):
        self.s, self.ctx, self.a, self.L = s, ctx, a, ctx.L
        self.ad = ad  # SxSampleAdapt: propose / leap / decide then go through their *_adapt forms,
        self.mt = mt  # with SxSampleMetric behind it through their *_metric forms
        Cn, n = s.chains, s.ndim
        self.hmc = s.method == _lib.SX_SAMPLE_HMC
        self.prop = ctx.empty((Cn, n))
        self.pmom = self.k0 = None
        if self.hmc:
            self.pmom = ctx.empty((Cn, n))
            self.k0 = ctx.empty((Cn,))
            if s.gradient is None:
                self.chunk = fd_axes_per_chunk(Cn, n)
                self.W = ctx.empty((self.chunk, 2, Cn, n))
                self.G = ctx.empty((Cn, n))

    def call(self, name, *args):
        _lib.check(getattr(self.L, name)(C.byref(self.a), *args, self.ctx.stream_ptr), name)

    def adapting(self, name, *args):
        if self.ad is None:
            return self.call(name, *args)
        if self.mt is None:
            return self.call(name + "_adapt", C.byref(self.ad), *args)
        self.call(name + "_metric", C.byref(self.ad), C.byref(self.mt), *args)

    def gradient(self):
        s, ptr = self.s, _device.ptr
        if s.gradient is not None:
            return s.gradient(self.ctx, self.prop)
        for axis0 in range(0, s.ndim, self.chunk):
            naxes = min(self.chunk, s.ndim - axis0)
            self.call("sx_sample_fd_rows", ptr(self.prop), axis0, naxes, ptr(self.W))
            fW = s.external(self.ctx, self.W[:naxes].reshape(-1, s.ndim))  # one call for the chunk's 2 * naxes * C rows
            self.call("sx_sample_fd_gradient", ptr(fW), axis0, naxes, ptr(self.G))
        return self.G

    def sample(self, i):
        s, ptr = self.s, _device.ptr
        self.adapting("sx_sample_propose", i, ptr(self.prop), ptr(self.pmom), ptr(self.k0))
        if self.hmc and i > 0:
            for g in range(s.nleap + 2):
                G = self.gradient()
                self.adapting("sx_sample_leap", 0.5 if g in (0, s.nleap + 1) else 1.0, int(g <= s.nleap), ptr(self.prop),
                              ptr(self.pmom), ptr(G))
        f = s.external(self.ctx, self.prop)
        self.adapting("sx_sample_decide", i, ptr(self.prop), ptr(f), ptr(self.pmom), ptr(self.k0))


def chain_args(ctx, s, rows, chains=None, x0=None, draws=None):
    """``(dev, a)``: the per-chain device arrays of a run of ``s`` (a Setup, or anything with its fields) and the
    SxSampleArgs that points at them, on the current stream.  ``rows``: the rows of xall / funall to keep per chain on the
    device, None for neither.  ``chains``: the length of the per-chain arrays when it is not ``s.chains`` -- the replicas of a
    tempered run, whose xall / funall stay one per ladder.  ``x0``: the initial point(s) as the kernels read them, (ndim,)
    for all or one row per chain.  ``draws``: (normals, logu) of the numpy-legacy stream, which the kernels then read
    (SX_RNG_HOST) instead of making their own."""
    t = _device.torch()
    Cn, n = s.chains if chains is None else chains, s.ndim
    dev = {name: ctx.empty((Cn, n)) for name in ("cur", "xbest")}
    dev.update({name: ctx.empty((Cn,)) for name in ("fcur", "facc", "fmin")})
    dev.update({name: ctx.empty((Cn,), dtype=t.int64) for name in ("iacc", "imin", "nacc", "nfeas")})
    if rows is not None:
        dev["xall"] = ctx.empty((s.chains, rows, n))
        dev["funall"] = ctx.empty((s.chains, rows))
    for name in ("lower", "upper", "step"):
        dev[name] = ctx.upload(getattr(s, name))
    if x0 is not None:
        dev["x0"] = ctx.upload(x0)
    if draws is not None:
        dev["normals"], dev["logu"] = (ctx.upload(d) for d in draws)
    a = _lib.SxSampleArgs()
    for name in ("cur", "fcur", "facc", "fmin", "xbest", "iacc", "imin", "nacc", "nfeas", "x0", "xall", "funall",
                 "lower", "upper", "step", "normals", "logu"):
        setattr(a, name, _device.ptr(dev.get(name)))
    a.C, a.maxiter = Cn, s.maxiter
    a.x0_stride = n if (x0 is not None and x0.ndim == 2) else 0
    a.n, a.fun_id, a.method = n, s.fun_id, s.method
    a.rng = _lib.SX_RNG_HOST if draws is not None else _lib.SX_RNG_PHILOX
    a.reject, a.k, a.nleap, a.jac, a.fd_step = int(s.reject), s.k, s.nleap, s.jac, s.fd_step
    a.key0, a.key1 = s.key
    return dev, a


def metric_args(ctx, dev, chains, ndim, start, ends):
    """The SxSampleMetric of a run whose windows are (start, ends[0]], (ends[0], ends[1]], ...; its device arrays go into
    ``dev`` (the launch that generates sample 0 writes them)."""
    mt = _lib.SxSampleMetric()
    dev["sbase"] = ctx.empty((chains,))
    dev.update({name: ctx.empty((chains, ndim)) for name in ("m", "mean", "M2")})
    for name in ("sbase", "m", "mean", "M2"):
        setattr(mt, name, _device.ptr(dev[name]))
    mt.nwin, mt.win_start = len(ends), start
    for j, end in enumerate(ends):
        mt.win_end[j] = end
    return mt


def run(s):
    L = _lib.lib()
    legacy = s.rng == "numpy-legacy"
    Cn, n, m = s.chains, s.ndim, s.maxiter
    stream = draws = None
    x0 = s.x0
    if legacy:
        stream, x0, *draws = _legacy_draws(s)
    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        on_device_all = s.return_all and s.callback is None
        rows = m if s.adapt is None else s.adapt.rows  # (burn / thin: the rows of xall / funall per chain)
        dev, a = chain_args(ctx, s, rows if on_device_all else None, x0=x0, draws=draws)
        ad = None
        if s.adapt is not None:
            ad = _lib.SxSampleAdapt()
            if s.adapt.warmup > 0:
                dev.update({name: ctx.empty((Cn,)) for name in ("scale", "hbar", "logsbar")})
                dev["nacc_warm"] = ctx.empty((Cn,), dtype=t.int64)
            for name in ("scale", "hbar", "logsbar", "nacc_warm"):
                setattr(ad, name, _device.ptr(dev.get(name)))
            ad.warmup, ad.rec_start, ad.rec_rows, ad.target = s.adapt.warmup, s.adapt.burn, rows, s.adapt.target
            ad.rec_every = min(s.adapt.thin, m)  # (the same rows; the library takes rec_every < 2^31)
        mt = None
        if s.adapt is not None and s.adapt.windows is not None:  # metric="diag": per-axis scales learnt in these windows
            mt = metric_args(ctx, dev, Cn, n, *s.adapt.windows)

        def host(name):
            return dev[name].cpu().numpy()

        def launch(i, steps):
            if ad is None:
                _lib.check(L.sx_sample_run(C.byref(a), i, steps, ctx.stream_ptr), "sx_sample_run")
            elif mt is not None:
                _lib.check(L.sx_sample_run_metric(C.byref(a), C.byref(ad), C.byref(mt), i, steps, ctx.stream_ptr),
                           "sx_sample_run_metric")
            else:
                _lib.check(L.sx_sample_run_adapt(C.byref(a), C.byref(ad), i, steps, ctx.stream_ptr), "sx_sample_run_adapt")

        if s.external is not None:
            advance = _Unfused(s, ctx, a, ad, mt).sample
        else:
            def advance(i):
                launch(i, 1)

        if s.callback is None:
            if s.external is not None:
                for i in range(m):
                    advance(i)
            else:  # the whole run is one launch
                launch(0, m)
            xall = host("xall") if on_device_all else None
            funall = host("funall") if on_device_all else None
        else:
            # one launch per sample; the state the callback sees is assembled as the reference does (mcmc/_mcmc.py:97-102
            # and :142-153, hmc/_hmc.py:128-133 and :174-185): x / fun = the best ACCEPTED sample so far (the first one
            # while there is none), nit and accept_ratio over the samples generated so far, xall / funall WITHOUT the newest
            xall = np.empty((Cn, m, n))
            funall = np.empty((Cn, m))
            for i in range(m):
                advance(i)
                xall[:, i] = host("cur")
                funall[:, i] = host("fcur")
                iacc = host("iacc")
                facc_now = funall[np.arange(Cn), iacc]
                b = int(np.argmin(facc_now))
                state = SampleResult(x=xall[b, iacc[b]], fun=facc_now[b], nit=i + 1,
                                     accept_ratio=1.0 if i == 0 else int(host("nacc").sum()) / (Cn * (i + 1)))
                if s.return_all:
                    upto = max(i, 1)
                    if s.adapt is not None:  # the recorded rows among the samples before the newest
                        upto = s.adapt.recorded[s.adapt.recorded < upto]
                    else:
                        upto = slice(0, upto)
                    state.update({"xall": xall[0, upto] if Cn == 1 else xall[:, upto],
                                  "funall": funall[0, upto] if Cn == 1 else funall[:, upto]})
                s.callback(xall[0, i] if Cn == 1 else xall[:, i], state)
            if s.adapt is not None:
                xall, funall = xall[:, s.adapt.recorded], funall[:, s.adapt.recorded]
        ctx.sync()
        nacc, nfeas = host("nacc"), host("nfeas")
        mcmc = s.method == _lib.SX_SAMPLE_MCMC
        fbest = host("facc" if mcmc else "fmin")
        xbest = host("xbest")
        warm = s.adapt is not None and s.adapt.warmup > 0
        if warm:
            scale, nacc_warm = host("scale"), host("nacc_warm")
        if mt is not None:
            metric = host("m")
    if stream is not None:
        stream.sync_back()  # numpy's global stream is where the reference would leave it
    b = int(np.argmin(fbest))  # (numpy's rule: the first NaN, else the first minimum; all inf: chain 0)
    res = SampleResult(x=xbest[b], fun=fbest[b], nit=m, accept_ratio=int(nacc.sum()) / (Cn * m))
    if not mcmc:
        grad_calls = 2 * n * (s.nleap + 2) if s.jac == _lib.SX_JAC_FINITE_DIFF else 0
        res["nfev"] = Cn * (1 + (m - 1) * grad_calls) + 2 * int(nfeas.sum())
    if s.reject:
        res["nreject"] = Cn * (m - 1) - int(nfeas.sum())  # proposals that left the box
    if Cn > 1:
        res["accept_ratios"] = nacc / m
    if warm:
        after = m - 1 - s.adapt.warmup  # samples generated with the frozen step
        sampling = (nacc - nacc_warm) / after if after > 0 else np.zeros(Cn)
        res["stepsizes"] = scale[0] if Cn == 1 else scale
        res["accept_ratios_sampling"] = sampling[0] if Cn == 1 else sampling
        res["warmup"] = s.adapt.warmup
    if mt is not None:
        res["metric"] = metric[0] if Cn == 1 else metric
        res["metric_windows"] = s.adapt.windows[1]
    if s.return_all:
        res["xall"] = xall[0] if Cn == 1 else xall
        res["funall"] = funall[0] if Cn == 1 else funall
    return res
