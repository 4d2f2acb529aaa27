"""The run drivers CMA-ES (_cmaes.py) and VD-CMA (_vdcma.py) share, in the manner of _population.py: what the two
front ends check, the device-resident run (`_DeviceRun`: the host enqueues generations and looks at the 128-byte state
record now and then) and the host-driven run (`_HostRun`: candidates and objective on the device, ranking, model and
stopping rules on the host).  Constructing a run builds its state; `run()` carries out the generation loop.  What
differs between the methods is left to class attributes and hooks of the subclasses (`_DeviceRun`: `Args`, `ENTRY`,
`GATHERED`, `_model`, `_scalar_args`, `_init_state`, `_look_cap`, `_begin`, `_enqueue`, `_look`, `_after_look`,
`_last_state`, `_check_status`; `_HostRun`: `_setup`, `_sample`, `_update`)."""
import ctypes as C
import os

import numpy as np

from .. import _device, _lib, _rng
from . import _common, _runs
from ._helpers import OptimizeResult


def check_arguments(bounds, x0, sigma, muperc, constraints, callback, runs=None):
    """What both front ends refuse (cmaes/_cmaes.py:142-160, vdcma/_vdcma.py:143-161).  Returns ``sigma``: as given, or --
    a sequence with ``runs=R``, one step size per run -- as an (R,) array."""
    if x0 is not None:
        if np.ndim(x0) != 1 or len(x0) != len(bounds):
            raise ValueError()
    sigma = _runs.per_run("sigma", sigma, runs, positive=True)
    if not 0.0 < muperc <= 1.0:
        raise ValueError()
    if constraints not in (None, "Penalize"):
        raise KeyError(constraints)
    if callback is not None and not hasattr(callback, "__call__"):
        raise ValueError()
    return sigma


def device_loop_serves(fun_id, rng, n, popsize, constraints):
    """Nothing the host has to COMPUTE between generations: Philox draws, a factory objective and -- with Penalize -- a
    spread history (20 + 3 n / P entries and the new one) that fits the 256 slots of the device workspace.
    SX_CMA_LOOP=host: the host-driven loop (tests, tools/bench_c4.py)."""
    return (rng == "philox" and isinstance(fun_id, int) and os.environ.get("SX_CMA_LOOP", "") != "host"
            and (constraints is None or 20.0 + 3.0 * n / int(popsize) + 1.0 <= 256.0))


def selection_weights(n, P, muperc):
    """mu, w, mueff, cc (cmaes/_cmaes.py:184-196, vdcma/_vdcma.py:185-193)."""
    mu = int(muperc * P)
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    w /= w.sum()
    mueff = w.sum() ** 2 / np.square(w).sum()
    cc = (4.0 + mueff / n) / (n + 4.0 + 2.0 * mueff / n)
    return mu, w, mueff, cc


def look_generations(maxiter, cap, every):
    """The generations after which the host reads the state record: 1, 2, 4, ... `cap` generations apart (`every`:
    always 1 -- a callback sees every generation, and the ranks of a sharded run must stop enqueueing collectives at the
    same one), and the last.  A matter of speed only: generations enqueued after the stop are no-ops."""
    gens, gen, look = [], 0, 1
    while gen < maxiter:
        gen = min(gen + look, maxiter)
        gens.append(gen)
        if not every and look < cap:
            look *= 2
    return gens


class _DeviceRun:
    """A run whose every per-generation step is on the device (csrc/sx_cma_loop.hip, csrc/sx_vd_loop.hip).  Draws: Philox
    normals keyed by (seed, generation, row).  ``buffers`` / ``args`` are the device state and the argument record of the
    generation entry points; ``step`` enqueues single generations from a state of the caller's choosing (tests, tools)."""

    LOOK = 16
    NAME = Args = ENTRY = None  # the method's name in messages, its argument record, its generation entry point
    GATHERED = ()               # sharded: the buffers every rank fills its rows of, in the order they are gathered

    def __init__(self, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, seed, return_all=False,
                 verbosity=1.0, penalize=False, workers=1, callback=None):
        ctx = self.ctx = _device.Context()
        t = _device.torch()
        n = self.n = len(lower)
        self.P, self.maxiter, self.muperc = P, maxiter, muperc
        self.penalize, self.return_all, self.callback = penalize, return_all, callback
        self.world, self.row0, self.Pl = None, 0, P
        if workers != 1:
            from ..parallel import require_world

            self.world = require_world(workers)
            self.row0, self.Pl = self.world.shard(P)  # blocks of ceil(P / workers) rows, the last rank short
        with t.cuda.stream(ctx.stream):
            init = self.init = _rng.make_init_stream("philox", seed)  # (freed with the run, after its last generation)
            key0, key1 = _rng.philox_key(seed)
            xm, xstd = self.xm, self.xstd = 0.5 * (upper + lower), 0.5 * (upper - lower)
            xmean = init.uniform(-1.0, 1.0, n) if x0 is None else (np.asarray(x0, dtype=np.float64) - xm) / xstd
            Z = ctx.empty((P, n))
            own = self._model(init)  # (the method's buffers, the candidates among them; sets self.mu, self.w)
            keep = self.buffers = dict(
                Z=Z, fit=ctx.empty((P,)), xmean=ctx.upload(xmean), xold=ctx.zeros((n,)), pc=ctx.zeros((n,)),
                w=ctx.upload(self.w), besthist=ctx.zeros((maxiter,)), xm=ctx.upload(xm), xstd=ctx.upload(xstd),
                xbest=ctx.zeros((n,)), order=ctx.empty((P,), dtype=t.int64), **own)
            if penalize:  # cmaes/_constraints.py:4-82 on the device: weights 0, spread history [1.0], both phase flags as at :213-215
                pw = np.zeros(2 * n + P + 256 + 4)
                pw[2 * n + P] = 1.0
                pw[2 * n + P + 256: 2 * n + P + 259] = (1.0, 0.0, 1.0)
                keep["pen_ws"] = ctx.upload(pw)
                keep["pen_order"] = ctx.empty((P,), dtype=t.int64)
            nout = int(np.ceil(verbosity * P)) if return_all else 0
            if return_all:  # device-side history slabs, read back once at the end
                keep["hist_x"] = ctx.empty((maxiter, max(1, nout), n))
                keep["hist_f"] = ctx.empty((maxiter, max(1, nout)))
            st = _lib.SxCmaState(it=0, nfev=0, best_row=0, fbest=0.0, sigma=sigma, sigma_next=sigma, tmp_coef=0.0,
                                 psnorm=0.0, status=_lib.SX_STATUS_NONE, done=0, stop_it=0)
            self._init_state(st)
            self._state0 = st
            keep["state"] = ctx.upload(np.frombuffer(bytes(st), dtype=np.float64))
            a = self.args = self.Args(**{k: _device.ptr(v) for k, v in keep.items()})
            a.P, a.hist_rows, a.n, a.mu, a.fun_id, a.maxiter = P, nout, n, self.mu, fun_id, maxiter
            a.ilim = int(10.0 + 30.0 * n / P)
            a.xtol, a.ftol, a.insigma, a.key0, a.key1 = xtol, ftol, sigma, key0, key1
            self._scalar_args(a)
            if self.world is not None:  # this rank's rows of what is gathered
                self._local = [ctx.empty((self.Pl,) + tuple(keep[k].shape[1:])) for k in self.GATHERED]
        self._res = None

    # ---- hooks ----
    def _model(self, init):
        """The method's own device buffers by their names in `Args`, the candidates ``arx`` among them; sets ``self.mu``
        and ``self.w``.  `init` is the stream the initial mean came from."""
        raise NotImplementedError

    def _scalar_args(self, a):
        """The method's own scalars of the argument record."""
        raise NotImplementedError

    def _init_state(self, st):
        """The method's own entries of the initial state record."""

    def _look_cap(self):
        """Most generations between two looks."""
        return self.LOOK

    def _begin(self):
        """Set-up of the loop that a run driven by `step` does not need."""

    def _enqueue(self, gen):
        """Enqueue generation `gen`.  A method that had to look at the device to do so returns the state record it saw
        (the loop then does not look again after this generation)."""
        self._generation(gen)

    def _look(self):
        """The state record, behind one synchronisation."""
        return self.read_state()

    def _after_look(self):
        """What a look tells the method about the generations to come."""

    def _last_state(self, state):
        """The record the result is made from."""
        return state

    def _check_status(self, state):
        """The method's own end-of-run faults."""

    # ---- one generation ----
    def _call(self, entry, *args):
        _lib.check(getattr(self.ctx.L, entry)(C.byref(self.args), *args, self.ctx.stream_ptr), entry)

    def _generation(self, gen, *how):
        """One GPU: one call.  Sharded: own candidates, one gather of each GATHERED buffer, the model update replicated
        on every rank."""
        if self.world is None:
            return self._call(self.ENTRY, gen, *how)
        self._call(self.ENTRY + "_stage", gen, *how, 0, self.row0, self.Pl, *(_device.ptr(loc) for loc in self._local))
        for loc, k in zip(self._local, self.GATHERED):
            self.world.all_gather_rows(loc, self.buffers[k])
        self._call(self.ENTRY + "_stage", gen, *how, 1, 0, 0, *(None for _ in self._local))

    def step(self, gen, *how):
        """Enqueue generation ``gen`` on its own (CMA-ES: ``how`` = 0 no decomposition, 1 cold, 2 started from the
        current B)."""
        with _device.torch().cuda.stream(self.ctx.stream):
            self._call(self.ENTRY, int(gen), *(int(h) for h in how))

    def read_state(self):
        return _lib.SxCmaState.from_buffer_copy(self.buffers["state"].cpu().numpy().tobytes())

    # ---- the loop ----
    def _show(self, gen, state):
        """What the reference hands its callback (cmaes/_cmaes.py:333-343, vdcma/_vdcma.py:413-423): all candidates (the
        clipped ones with Penalize), un-standardised, and the best of them; with return_all the history so far (copied
        slab by slab)."""
        keep, t = self.buffers, _device.torch()
        if self._cb_pin is None:
            self._cb_pin = t.empty((self.P, self.n), dtype=t.float64).pin_memory()
        self._cb_pin.copy_(keep["arx"])
        rows = self._cb_pin.numpy()
        Xs = np.multiply(np.clip(rows, -1.0, 1.0) if self.penalize else rows, self.xstd)  # (a new array every generation)
        Xs += self.xm
        cres = OptimizeResult(x=Xs[int(state.best_row)].copy(), fun=float(state.fbest), nfev=gen * self.P, nit=gen)
        if self.return_all:
            if self._cb_hist is None:
                self._cb_hist = (np.empty(tuple(keep["hist_x"].shape)), np.empty(tuple(keep["hist_f"].shape)))
            self._cb_hist[0][gen - 1] = keep["hist_x"][gen - 1].cpu().numpy()
            self._cb_hist[1][gen - 1] = keep["hist_f"][gen - 1].cpu().numpy()
            cres.update({"xall": self._cb_hist[0][:gen], "funall": self._cb_hist[1][:gen]})
        self.callback(Xs, cres)

    def run(self):
        """Enqueue generations until a look finds the run stopped; returns the result."""
        keep, P = self.buffers, self.P
        self._cb_pin = self._cb_hist = None
        with _device.torch().cuda.stream(self.ctx.stream):
            looks = set(look_generations(self.maxiter, self._look_cap(), self.world is not None or self.callback is not None))
            state = self._state0
            self._begin()
            for gen in range(1, self.maxiter + 1):
                seen = self._enqueue(gen)
                if seen is not None:  # (the method looked while it enqueued)
                    state = seen
                elif gen in looks:
                    state = self._look()
                    if self.callback is not None:
                        self._show(gen, state)
                    if not state.done:
                        self._after_look()
                if state.done:
                    break
            state = self._last_state(state)
            if not state.done:  # cannot happen: generation maxiter sets status -1
                raise RuntimeError(f"{self.NAME} device loop ended without a status")
            self._check_status(state)
            nit = int(state.stop_it)
            self._res = OptimizeResult(x=keep["xbest"].cpu().numpy(), success=state.status >= 0, status=int(state.status),
                                       message=_common.messages[int(state.status)], fun=float(state.fbest),
                                       nfev=nit * P, nit=nit)
            if self.return_all:
                self._res.update({"xall": keep["hist_x"][:nit].cpu().numpy(), "funall": keep["hist_f"][:nit].cpu().numpy()})
            self.ctx.sync()
        return self._res

    def result(self):
        return self._res if self._res is not None else self.run()


class _BoundaryWeights:
    """Host bookkeeping of constraints="Penalize" (cmaes/_constraints.py:33-76; state created at
    cmaes/_cmaes.py:213-215, 230-231): per-dimension penalty weights, the sliding history of fitness-spread
    estimates they are initialised from, and the two phase flags.  ``update`` takes the RAW fitness of the
    clipped candidates and returns ``weights / scale`` -- the vector the device multiplies the squared excess by."""

    def __init__(self, n):
        self.weights = np.zeros(n)
        self.spreads = np.ones(1)
        self.have_spread = False
        self.initial_phase = True

    def update(self, fit_raw, xmean, xold, sigma, diagC, mueff, it, P):
        n = xmean.size
        q25, q75 = np.percentile(fit_raw, [25.0, 75.0])
        spread = (q75 - q25) / n / diagC.mean() / sigma**2
        if spread == 0:
            spread = self.spreads[self.spreads > 0.0].min()
        elif not self.have_spread:
            self.spreads = np.empty(0)
            self.have_spread = True
        keep = self.spreads if self.spreads.size < 20 + (3.0 * n) / P else self.spreads[1:]
        self.spreads = np.append(keep, spread)
        outside = (xmean < -1.0) | (xmean > 1.0)
        if outside.any():
            if self.initial_phase:
                self.weights = np.full(n, 2.0002 * np.median(self.spreads))
                if self.have_spread and it > 2:
                    self.initial_phase = False
            # the reference measures the excess against a mean clipped on the UPPER side only (:52-53: the
            # second np.where starts again from xmean), so weights only ever grow for dimensions above +1
            excess = xmean - np.where(xmean > 1.0, 1.0, xmean)
            limit = 3.0 * max(1.0, np.sqrt(n / mueff)) * sigma * np.sqrt(diagC)
            grow = outside & (np.abs(excess) > limit) & (np.sign(excess) == np.sign(xmean - xold))
            self.weights = np.where(grow, self.weights * 1.2 ** min(1.0, mueff / 10.0 / n), self.weights)
        logd = np.log(diagC)
        return self.weights / np.exp(0.9 * (logd - logd.mean()))


def _stop_status(it, n, maxiter, xmean, xold, besthist, arfit, order, sigma, insigma, ilim, pc, xtol, ftol, diagC, B, D):
    """The ten ordered stopping rules of cmaes/_cmaes.py:360-434 (including the zero-padded history reads)."""
    axis = int(np.floor(np.mod(it, n)))
    sd = np.sqrt(diagC)
    fbest = arfit[order[0]]
    if it >= maxiter:
        return -1
    if np.linalg.norm(xold - xmean) <= xtol and fbest < ftol:
        return 0
    if fbest <= ftol:
        return 1
    if B is not None and (np.abs(0.1 * sigma * B[:, axis] * D[axis]) < 1.0e-10).all():  # VD-CMA passes no B, D
        return -2
    if (0.2 * sigma * sd < 1.0e-10).any():
        return -3
    if D is not None and D.max() > 1.0e7 * D.min():
        return -4
    if it >= ilim:
        window = besthist[it - ilim : it + 1]
        if window.max() - window.min() < 1.0e-10:
            return -5
    if (sigma * sd > 1.0e3 * insigma).any():
        return -6
    if it > 2:
        joined = np.append(arfit, besthist)
        if joined.max() - joined.min() < 1.0e-12:
            return -7
    if (sigma * np.append(np.abs(pc), sd.max()) < 1.0e-11 * insigma).all():
        return -8
    return None


class _HostRun:
    """A run the host drives (cmaes/_cmaes.py:226-343, vdcma/_vdcma.py:232-425): normals (the numpy-legacy stream,
    replicated on every rank, or in-kernel Philox keyed by the global row), candidates, objective and the Penalize excess
    on the device; ranking, the model (`_update`) and the stopping rules on the host.  The model's hooks keep
    ``xmean, xold, sigma, diagC, mueff`` current: the Penalize bookkeeping reads them before the update."""

    def __init__(self, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, return_all, verbosity,
                 callback, rng, seed, workers=1, penalize=False):
        self.penalize = penalize
        self.world = None
        if workers != 1:
            from ..parallel import require_world

            self.world = require_world(workers)
            self.world.shard(P)  # blocks of ceil(P / workers) rows, the last rank short
        self.fun_id, self.maxiter, self.P, self.n = fun_id, maxiter, P, len(lower)
        self.muperc, self.xtol, self.ftol = muperc, xtol, ftol
        self.return_all, self.callback, self.rng = return_all, callback, rng
        ctx, n = _device.Context(), self.n
        self.ctx = ctx
        t = _device.torch()
        with t.cuda.stream(ctx.stream):
            self.stream = _rng.make_init_stream(rng, seed)
            self.key = _rng.philox_key(seed) if rng == "philox" else (0, 0)
            # standardisation to [-1, 1]^n (cmaes/_cmaes.py:167-173)
            self.xm, self.xstd = 0.5 * (upper + lower), 0.5 * (upper - lower)
            self.d_xm, self.d_xstd = ctx.upload(self.xm), ctx.upload(self.xstd)
            self.xmean = (self.stream.uniform(-1.0, 1.0, n) if x0 is None
                          else (np.asarray(x0, dtype=np.float64) - self.xm) / self.xstd)
            self.xold = np.zeros(n)  # the reference reads an uninitialised array here in generation 1 (np.empty)
            self.sigma = self.insigma = sigma
            self.d_arx, self.d_fit = ctx.empty((P, n)), ctx.empty((P,))
            # this rank's candidates: rows [row0, row0 + Pl) of the generation (all of them on one GPU)
            self.row0, self.Pl = (0, P) if self.world is None else self.world.shard(P)
            self.d_Z = ctx.empty((self.Pl, n))
            self.d_arx_loc = self._local(self.d_arx)
            self.d_fit_loc = self._local(self.d_fit)
            self.gathered = [(self.d_arx_loc, self.d_arx), (self.d_fit_loc, self.d_fit)]  # (what every rank gets back, in order)
            self.h_Z = t.empty((P, n), dtype=t.float64).pin_memory() if rng == "numpy-legacy" else None
            if penalize:
                self.bweights = _BoundaryWeights(n)
                self.d_v, self.d_pen = ctx.empty((n,)), ctx.empty((P,))
                self.d_pen_loc = self._local(self.d_pen)
            if return_all:
                self.nout = int(np.ceil(verbosity * P))
                self.xall = np.empty((maxiter, max(1, self.nout), n))
                self.funall = np.empty((maxiter, max(1, self.nout)))
            self.besthist = np.zeros(maxiter)
            self.ilim = int(10.0 + 30.0 * n / P)
            self._setup()
        self._res = None

    # ---- hooks ----
    def _setup(self):
        """The model: ``mu, w, mueff, pc, diagC`` and the method's own host and device state."""
        raise NotImplementedError

    def _sample(self, it):
        """This rank's candidates of generation `it` from the normals in ``d_Z`` into ``d_arx_loc``."""
        raise NotImplementedError

    def _update(self, it, arfit, order):
        """The model update from the ranked generation; returns the ``B, D`` the stopping rules read (or None, None)."""
        raise NotImplementedError

    def _local(self, full):
        """This rank's rows of a gathered buffer (one GPU: the buffer itself)."""
        return full if self.world is None else self.ctx.empty((self.Pl,) + tuple(full.shape[1:]))

    def _put(self, dst, a):
        dst.copy_(_device.torch().from_numpy(np.ascontiguousarray(a)))

    def seen(self, rows):
        """What the caller sees of standardised candidates: with Penalize the clipped points
        (cmaes/_cmaes.py:238-256, 336-350), un-standardised."""
        return (np.clip(rows, -1.0, 1.0) if self.penalize else rows) * self.xstd + self.xm

    def _partial(self, it, arfit, order, **more):
        res = OptimizeResult(x=self.seen(self.d_arx[int(order[0])].cpu().numpy()), **more, fun=arfit[order[0]],
                             nfev=it * self.P, nit=it)
        if self.return_all:
            res.update({"xall": self.xall[:it], "funall": self.funall[:it]})
        return res

    def run(self):
        """Generations until a stopping rule fires; returns the result."""
        ctx, L, n, P, ptr = self.ctx, self.ctx.L, self.n, self.P, _device.ptr
        with _device.torch().cuda.stream(ctx.stream):
            it = 0
            while True:
                it += 1
                # ---- normals from the numpy-legacy stream or in-kernel Philox, then the method's candidates ----
                if self.rng == "numpy-legacy":
                    self.stream.randn(None, out=self.h_Z.numpy())  # P x randn(n), row by row == one block (cmaes/_cmaes.py:234)
                    self.d_Z.copy_(self.h_Z[self.row0 : self.row0 + self.Pl], non_blocking=True)
                else:
                    _lib.check(L.sx_cmaes_normals(ptr(self.d_Z), self.Pl, n, self.row0, it, *self.key, ctx.stream_ptr),
                               "sx_cmaes_normals")
                self._sample(it)
                # ---- evaluate: fun(unstandardize(x)) fused (cmaes/_cmaes.py:173, 258); with Penalize the candidates are
                # clipped to the box before the objective (cmaes/_constraints.py:29-31) ----
                _common.evaluate_rows(ctx, self.fun_id, self.d_arx_loc, n, self.d_fit_loc, xm=self.d_xm, xstd=self.d_xstd,
                                      clip=self.penalize)
                if self.world is not None:  # every rank gets all candidates and fitness values back
                    for loc, full in self.gathered:
                        self.world.all_gather_rows(loc, full)
                arfit = self.d_fit.cpu().numpy()
                if self.penalize:
                    # host: boundary weights from the raw fitness spread (:33-76); device: weighted squared excess (:79)
                    v = self.bweights.update(arfit, self.xmean, self.xold, self.sigma, self.diagC, self.mueff, it, P)
                    if v.any():
                        self._put(self.d_v, v)
                        _common.penalty_rows(ctx, self.fun_id, self.d_arx_loc, n, self.d_xm, self.d_xstd, self.d_v,
                                             self.d_fit_loc, self.d_pen_loc)
                        if self.world is not None:
                            self.world.all_gather_rows(self.d_pen_loc, self.d_pen)
                        arfit = arfit + self.d_pen.cpu().numpy()
                if self.return_all:
                    if self.nout > 0:
                        self.xall[it - 1] = self.seen(self.d_arx[: self.nout].cpu().numpy())
                        self.funall[it - 1] = arfit[: self.nout]
                    else:
                        k = int(arfit.argmin())
                        self.xall[it - 1] = self.seen(self.d_arx[k].cpu().numpy())
                        self.funall[it - 1] = arfit[k]
                # ---- rank (cmaes/_cmaes.py:272), the method's model update, the stopping rules ----
                order = np.argsort(arfit)
                self.besthist[it - 1] = arfit[order[0]]
                B, D = self._update(it, arfit, order)
                status = _stop_status(it, n, self.maxiter, self.xmean, self.xold, self.besthist, arfit, order, self.sigma,
                                      self.insigma, self.ilim, self.pc, self.xtol, self.ftol, self.diagC, B, D)
                if self.callback is not None:
                    res = self._partial(it, arfit, order)
                    self.callback(self.seen(self.d_arx.cpu().numpy()), res)
                if status is not None:
                    break
            self._res = self._partial(it, arfit, order, success=status >= 0, status=status, message=_common.messages[status])
            if self.rng == "numpy-legacy":
                self.stream.sync_back()
            ctx.sync()
        return self._res

    def result(self):
        return self._res if self._res is not None else self.run()
