"""VD-CMA front end + model for ``backend="hip"``; the generation loops are the shared ones of _evolution.py.

Reference: stochopy/optimize/vdcma/_vdcma.py:12-141 (``minimize``) and :144-425 (``vdcma`` loop), :428-460
(the moment and natural-gradient helpers); stopping rules shared with CMA-ES (cmaes/_cmaes.py:360-434 without
B and D).  SURVEY.md section 8f rank 3: the covariance model is D (I + v v^T) D, so a generation is O(P n):

* on the device (csrc/sx_cmaes.hip ``vd_sample_kernel``, csrc/sx_core.hip): the P candidates
  ``y = d o (z + (sqrt(1+|v|^2)-1)(z.vn) vn)``, ``x = xmean + sigma y`` (one wavefront each, normals from the
  numpy-legacy stream or in-kernel Philox), the objective with fused un-standardisation and -- with
  ``constraints="Penalize"`` -- the clipping and the weighted squared excess (shared with CMA-ES);
* on the host, as in the reference: ranking, the weighted sums over the mu selected rows (moments p, q of
  :428-444), the natural-gradient step for v and d (:447-460), step size, stopping rules -- O(mu n) numpy.

``workers > 1``: candidates sharded by rows like CMA-ES (one all-gather of y, x and the fitness per generation).  The sharded
run is the one-GPU run bit for bit for models of up to 2048 coordinates.  Longer models (csrc/sx_wide.hip): on one GPU the
candidates kernel leaves t_k = sum(yd * vn) as a by-product, with yd the step BEFORE it is rounded through y = d * yd; the
sharded run forms t_k from the gathered y as (y / d) . vn (csrc/sx_vd_loop.hip vd_t_kernel, what the oracle does): the two
differ in the last bits of every t_k, so there the sharded run follows the one-GPU run to rounding, not bit for bit.
"""

import os

import numpy as np

from .. import _device, _lib, _rng
from . import _common, _evolution, _runs
from ._helpers import register

__all__ = ["minimize"]


def minimize(
    fun,
    bounds,
    x0=None,
    args=(),
    maxiter=100,
    popsize=10,
    sigma=0.1,
    muperc=0.5,
    seed=None,
    xtol=1.0e-8,
    ftol=1.0e-8,
    constraints=None,
    workers=1,
    backend=None,
    return_all=False,
    verbosity=1.0,
    callback=None,
    rng=None,
    host_workers=None,
    host_backend=None,
    runs=None,
):
    """Minimize an objective function using VD-CMA on MI355X (reference vdcma/_vdcma.py:12-30).

    ``runs=R`` (R >= 2) performs R independent runs with these settings in ONE kernel launch, one workgroup per run
    (csrc/sx_vd_runs.hip): run r is the run of ``seed + r`` (``seed`` an integer) or of ``seed[r]`` (a sequence of R
    integers) with ``rng="philox"`` -- the same draws, the same arithmetic up to the order of its sums; ``x0`` is ``None``
    (every run draws its initial mean as the single run of its seed does), one ``(n,)`` point for all runs or ``(R, n)``; the
    initial direction of run r is drawn right after its mean, as the single run draws it.  The result describes the best run
    (``np.argmin`` over the runs' ``fun``; ``run`` is its index, ``nfev`` the sum over all runs) and carries ``xs``, ``funs``,
    ``nits``, ``statuses`` and ``sigmas`` (the final step sizes) per run.  With ``runs=R``, ``sigma`` may be a sequence of R
    values, one per run (a sweep: run r starts from ``sigma[r]``, which is also what its stopping rules -6 and -8 compare
    with, as in the single run); the result then has ``sweep``, the dict ``{"sigma": the (R,) array used}``.  Needs
    ``rng="philox"``, a factory objective, one
    GPU, no callback, no ``return_all``, ``constraints=None``, ``ndim >= 6`` and a shape that fits one workgroup's LDS
    (``sx_vd_runs_lds_bytes``: popsize 10 up to ndim 512 and beyond)."""
    batched_runs = _runs.batched(runs)
    fun_id = _common.resolve_objective(fun, args, workers, backend, host_workers, host_backend)
    lower, upper = _common.as_bounds(bounds)
    if batched_runs and x0 is not None and np.ndim(x0) == 2:  # a point per run
        if np.shape(x0) != (runs, len(bounds)):
            raise ValueError(f"x0 of shape {np.shape(x0)} with runs={runs}: expected ({len(bounds)},) for all runs or "
                             f"({runs}, {len(bounds)})")
        sigma = _evolution.check_arguments(bounds, None, sigma, muperc, constraints, callback, runs)
    else:
        sigma = _evolution.check_arguments(bounds, x0, sigma, muperc, constraints, callback, runs)
    _common.resolve_backend(backend, fun_id)
    rng = _common.resolve_rng(rng)
    if batched_runs:
        return _minimize_runs(int(runs), fun_id, lower, upper, x0, int(maxiter), int(popsize), _runs.setting(sigma),
                              float(muperc), float(xtol), float(ftol), seed, rng, constraints, workers, return_all,
                              callback)
    workers = _common.resolve_workers(workers, fun_id)
    if _evolution.device_loop_serves(fun_id, rng, len(lower), popsize, constraints):
        # the whole loop (and the history) stays on the device -- since round 3 including constraints="Penalize"
        # (boundary-weight bookkeeping shared with CMA-ES: cma_penalty_kernel) and workers > 1 (own candidates, one gather of
        # steps / candidates / fitness, the O(n) model update replicated); a callback is served from this loop too (the host
        # then looks at every generation).
        # Wide models whose candidates nobody else wants (no callback, history, Penalize, sharding): x = xmean + sigma y is
        # not kept -- the moments kernel forms it again from y, bit for bit (sx_vd_args.arx NULL): a quarter of a
        # generation's memory traffic
        keep_x = not (len(lower) > _lib.NARROW_DIM and callback is None and not return_all and constraints is None
                      and workers == 1 and os.environ.get("SX_VD_KEEP_X", "0") != "1")
        return _VdDeviceRun(fun_id, lower, upper, x0, int(maxiter), int(popsize), float(sigma), float(muperc),
                            float(xtol), float(ftol), seed, bool(return_all), float(verbosity),
                            penalize=constraints == "Penalize", workers=workers, callback=callback, keep_x=keep_x).run()
    return _VdRun(fun_id, lower, upper, x0, int(maxiter), int(popsize), float(sigma), float(muperc), float(xtol),
                  float(ftol), bool(return_all), float(verbosity), callback, rng, seed, workers=workers,
                  penalize=constraints == "Penalize").run()


def _strategy_constants(n, P, muperc):
    """Selection weights and learning rates (vdcma/_vdcma.py:185-199)."""
    mu, w, mueff, cc = _evolution.selection_weights(n, P, muperc)
    cfactor = (n - 5.0) / 6.0
    c1 = cfactor * 2.0 / ((n + 1.3) ** 2 + mueff)
    cmu = min(1.0 - c1, cfactor * 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((n + 2.0) ** 2 + mueff))
    return mu, w, mueff, cc, c1, cmu


RUNS_MIN_DIM = 6  # runs > 1: below, the reference's learning rates c1, cmu are zero or negative (cfactor = (n - 5) / 6)


def _minimize_runs(R, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, seed, rng, constraints, workers,
                   return_all, callback):
    """``runs=R``: R independent runs, one workgroup each, one launch (csrc/sx_vd_runs.hip).  Everything that can be
    refused is refused before the device is touched."""
    n = len(lower)
    _runs.refuse_common(rng, fun_id, workers, callback, return_all)
    _runs.refuse_constraints(constraints)
    seeds = _runs.seeds_of(R, seed)
    _runs.refuse_maxiter(maxiter)
    if n < RUNS_MIN_DIM:
        raise ValueError(f"runs > 1 with method='vdcma' needs ndim >= {RUNS_MIN_DIM} (ndim = {n}): below, the reference's "
                         "learning rates c1 and cmu are zero or negative (cfactor = (ndim - 5) / 6) and the model never "
                         "learns; method='cmaes' with runs serves ndim <= 32 properly")
    lds = int(_lib.lib().sx_vd_runs_lds_bytes(P, n)) if P >= 1 else -1
    mu = int(muperc * P)
    if lds < 0 or mu < 1:
        raise ValueError(f"runs > 1 keeps a run's model and staging rows in one workgroup's LDS: popsize {P} x {n} variables "
                         f"(mu = {mu}) needs 2 <= popsize, mu >= 1, ndim <= {int(_lib.lib().sx_wide_from())} and at most "
                         "160 KiB")
    batch = _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol)
    batch.launch()
    return _runs.result(batch.fetch(), P, sigma=sigma)


def _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, outputs=()):
    """The batch of one sx_vd_runs_launch; ``outputs``: of the optional ones, ``"nfevs"`` and every run's final model --
    ``"xmeans"`` (standardised), ``"dvecs"``, ``"vvecs"``."""
    n, R = len(lower), len(seeds)
    mu, w, mueff, cc, c1, cmu = _strategy_constants(n, P, muperc)
    xm, xstd, given = _runs.standardised(lower, upper, x0, R)
    # what the single run of each seed draws on the host (_evolution._DeviceRun, _VdDeviceRun._model): its private legacy
    # stream gives the initial mean -- unless the caller gave one -- and right after it the initial direction
    xmean0, vvec0 = np.empty((R, n)) if given is None else given, np.empty((R, n))
    for r, s in enumerate(seeds):
        init = _rng.make_init_stream("philox", s)
        if given is None:
            xmean0[r] = init.uniform(-1.0, 1.0, n)
        vvec0[r] = init.randn(n) / np.sqrt(n)
    batch = _runs.Batch("sx_vd_runs_launch", _lib.SxVdRunsArgs(), seeds, P)
    a, ctx = batch.a, batch.ctx
    with batch.stream():
        batch.upload_keys()
        d_xmean0, d_vvec0, d_w = ctx.upload(xmean0), ctx.upload(vvec0), ctx.upload(w)
        d_std = ctx.upload_async(np.concatenate([xm, xstd]))
        batch.bind(xmean0=d_xmean0, vvec0=d_vvec0, w=d_w, xm=d_std[:n], xstd=d_std[n:],
                   work=ctx.empty((int(ctx.L.sx_vd_runs_workspace_bytes(R, maxiter)) // 8,)))
        vec = ((R, n), None)
        batch.outputs(n, {"nfevs": ((R,), _device.torch().int64), "xmeans": vec, "dvecs": vec, "vvecs": vec}, outputs,
                      extra=("sigmas",))
        own = batch.bind_sweep(sigma=sigma)
    _runs.set_model_scalars(a, n, mu, fun_id, maxiter, own["sigma"], xtol, ftol)
    a.mueff, a.cc, a.c1, a.cmu = mueff, cc, c1, cmu
    a.cs, a.ds, a.wsum = 0.3, float(np.sqrt(n)), float(w.sum())
    return batch


class _VdDeviceRun(_evolution._DeviceRun):
    """The reference's loop (vdcma/_vdcma.py:232-425) with every per-generation step on the device
    (csrc/sx_cma_loop.hip, sx_vdcma_generation).  The injection's normal row is "row P" of the generation's draws.
    ``keep_x=False``: the candidates ``buffers["arx"]`` are not stored (nobody but the moments kernel may want them then)."""

    NAME, Args, ENTRY, GATHERED = "VD-CMA", _lib.SxVdArgs, "sx_vdcma_generation", ("ary", "arx", "fit")

    def __init__(self, *args, keep_x=True, **kwargs):
        self.keep_x = keep_x
        super().__init__(*args, **kwargs)
        if not keep_x and (self.callback is not None or self.return_all or self.penalize or self.world is not None):
            raise ValueError("keep_x=False: the callback, the history, Penalize and the gathers all read the candidates")

    def _model(self, init):
        ctx, n, P = self.ctx, self.n, self.P
        mu, w, *self.constants = _strategy_constants(n, P, self.muperc)
        self.mu, self.w = mu, w
        vvec = init.randn(n) / np.sqrt(n)  # the first direction comes right after the initial mean in the stream
        with _common.host_blas_single_thread():  # (a threaded BLAS wakes 64+ spinning threads for this one dot product)
            self.norm_v2 = float(np.dot(vvec, vvec))
        norm_v = float(np.sqrt(self.norm_v2))
        own = dict(ary=ctx.empty((P, n)), dx=ctx.zeros((n,)), dvec=ctx.upload(np.ones(n)), vvec=ctx.upload(vvec),
                   vn=ctx.upload(vvec / norm_v), zinj=ctx.empty((n,)), dy=ctx.zeros((n,)),
                   mws=ctx.empty((((mu + 7) // 8) * 8 + 4 * 64 * n,)), mout=ctx.empty((4, n)))
        if self.keep_x:
            own["arx"] = ctx.empty((P, n))
        return own

    def _init_state(self, st):
        norm_v2 = self.norm_v2
        st.reserved[0], st.reserved[1], st.reserved[2] = 0.0, norm_v2, float(np.sqrt(norm_v2))  # ps, |v|^2, |v|
        st.reserved[3], st.reserved[4] = 0.0, float(np.sqrt(1.0 + norm_v2) - 1.0)            # injection off, coefficient

    def _scalar_args(self, a):
        a.mueff, a.cc, a.c1, a.cmu = self.constants
        a.cs, a.ds, a.wsum = 0.3, float(np.sqrt(self.n)), float(self.w.sum())

    def _check_status(self, state):
        if state.status == -99:  # csrc/sx_vd_loop.hip kVwFault
            raise RuntimeError("VD-CMA model update: a grid-wide wait of the single-launch chain ran out (is another kernel "
                               "holding the device?); SX_VD_CHAIN=0 runs the chain as one launch per phase")


def _moments(vn, norm_v2, y, w=None):
    """Moments p, q of the selected steps under the current model (vdcma/_vdcma.py:428-444)."""
    t = np.dot(y, vn)
    shrink = norm_v2 / (1.0 + norm_v2)
    if w is None:
        return y**2 - shrink * (t * y * vn) - 1.0, t * y - (0.5 * (t**2 + 1.0 + norm_v2)) * vn
    p = np.dot(w, y**2 - shrink * (t[:, None] * (y * vn)) - 1.0)
    q = np.dot(w, t[:, None] * y - np.outer(0.5 * (t**2 + 1.0 + norm_v2), vn))
    return p, q


def _natural_gradient(dvec, vn, vnn, norm_v, norm_v2, alpha, avec, bsca, invavnn, p, q):
    """Steps for v and d (vdcma/_vdcma.py:447-460)."""
    r = p - alpha / (1.0 + norm_v2) * ((2.0 + norm_v2) * q * vn - norm_v2 * np.dot(vn, q) * vnn)
    s = r / avec - bsca * np.dot(r, invavnn) / (1.0 + bsca * np.dot(vnn, invavnn)) * invavnn
    ngv = q / norm_v - alpha / norm_v * ((2.0 + norm_v2) * (vn * s) - np.dot(s, vnn) * vn)
    return ngv, dvec * s


class _VdRun(_evolution._HostRun):
    """The host-driven loop: candidates and the O(mu n) sums of the update on the device, the natural-gradient step for
    v and d, step size and stopping rules -- O(n) numpy -- on the host."""

    def _setup(self):
        ctx, n, P, t = self.ctx, self.n, self.P, _device.torch()
        self.mu, self.w, self.mueff, self.cc, self.c1, self.cmu = _strategy_constants(n, P, self.muperc)
        # dynamic state (:202-213); the first direction comes right after the initial mean in the stream
        self.inject, self.ps = False, 0.0
        self.dx, self.dvec, self.pc = np.zeros(n), np.ones(n), np.zeros(n)
        self.vvec = self.stream.randn(n) / np.sqrt(n)
        self._normalise()
        self.d_ary = ctx.empty((P, n))
        self.d_ary_loc = self._local(self.d_ary)
        self.gathered.insert(0, (self.d_ary_loc, self.d_ary))  # (the steps travel first)
        self.d_dvec, self.d_vn, self.d_xmean, self.d_dy = ctx.empty((n,)), ctx.empty((n,)), ctx.empty((n,)), ctx.empty((n,))
        self.d_zinj = ctx.empty((1, n))
        self.d_sel = ctx.empty((self.mu,), dtype=t.int64)
        self.d_w = ctx.upload(self.w)
        self.d_mws = ctx.empty((((self.mu + 7) // 8) * 8 + 4 * 64 * n,))
        self.d_mout = ctx.empty((4, n))

    def _normalise(self):
        self.norm_v2 = np.dot(self.vvec, self.vvec)
        self.norm_v = np.sqrt(self.norm_v2)
        self.vn = self.vvec / self.norm_v
        self.vnn = self.vn**2

    def _sample(self, it):
        """y = d o (z + (sqrt(1 + |v|^2) - 1)(z . vn) vn), x = xmean + sigma y (vdcma/_vdcma.py:236-248)."""
        ctx, L, n, P, ptr = self.ctx, self.ctx.L, self.n, self.P, _device.ptr
        dx, dvec, vvec, norm_v2 = self.dx, self.dvec, self.vvec, self.norm_v2
        dy = None
        if self.inject:  # mean-shift injection: rows 0 and 1 become +-dy (:241-247)
            ddx = dx / dvec
            mnorm = (ddx**2).sum() - np.dot(ddx, vvec) ** 2 / (1.0 + norm_v2)
            if self.rng == "numpy-legacy":
                zinj = self.stream.randn(n)
            else:  # "row P" of the generation's normals, one past the population
                _lib.check(L.sx_cmaes_normals(ptr(self.d_zinj), 1, n, P, it, *self.key, ctx.stream_ptr), "sx_cmaes_normals")
                zinj = self.d_zinj.cpu().numpy()[0]
            dy = np.linalg.norm(zinj) / np.sqrt(mnorm) * dx
            self._put(self.d_dy, dy)
        self._put(self.d_dvec, dvec)
        self._put(self.d_vn, self.vn)
        self._put(self.d_xmean, self.xmean)
        _lib.check(L.sx_vdcma_sample(ptr(self.d_Z), self.Pl, n, self.row0, ptr(self.d_dvec), ptr(self.d_vn),
                                     float(np.sqrt(1.0 + norm_v2) - 1.0), ptr(self.d_xmean), float(self.sigma),
                                     ptr(self.d_dy) if dy is not None else None, ptr(self.d_ary_loc), ptr(self.d_arx_loc),
                                     ctx.stream_ptr), "sx_vdcma_sample")
        self.diagC = (dvec * (1.0 + vvec * vvec)) * dvec  # diag of D (I + v v^T) D (:249-254)

    def _update(self, it, arfit, order):
        ctx, L, n, P, mu, ptr, t = self.ctx, self.ctx.L, self.n, self.P, self.mu, _device.ptr, _device.torch()
        w, mueff, cc, c1, cmu = self.w, self.mueff, self.cc, self.c1, self.cmu
        dvec, vvec, norm_v2, norm_v, vn, vnn, pc = self.dvec, self.vvec, self.norm_v2, self.norm_v, self.vn, self.vnn, self.pc
        # ---- every O(mu n) sum of the update on the device: the weighted means of the selected x and y and the rank-mu
        # moments (:289-295, :317, :331-339); four n-vectors come back ----
        self.d_sel.copy_(t.from_numpy(np.ascontiguousarray(order[:mu], dtype=np.int64)))
        _lib.check(L.sx_vdcma_moments(ptr(self.d_arx), ptr(self.d_ary), ptr(self.d_sel), ptr(self.d_w), mu, n, ptr(self.d_dvec),
                                      ptr(self.d_vn), float(norm_v2), ptr(self.d_mws), ptr(self.d_mout), ctx.stream_ptr),
                   "sx_vdcma_moments")
        wx, wy, p_mu_dev, q_mu_dev = self.d_mout.cpu().numpy()
        self.dx = wx - w.sum() * self.xmean
        self.xold = self.xmean.copy()
        self.xmean = self.xmean + self.dx
        # ---- step size from the rank gap of the injected pair (:298-306) ----
        if self.inject:
            gap = (np.where(order == 1)[0][0] - np.where(order == 0)[0][0]) / (P - 1.0)
            self.ps += 0.3 * (gap - self.ps)
            self.sigma *= np.exp(self.ps / np.sqrt(n))
            cond = self.ps < 0.5
        else:
            self.inject = True
            cond = True
        # ---- evolution path, model constants (:309-328) ----
        pc *= 1.0 - cc
        if cond:
            pc += np.sqrt(cc * (2.0 - cc) * mueff) * wy
        gamma = 1.0 / np.sqrt(1.0 + norm_v2)
        alpha = np.sqrt(norm_v2**2 + (1.0 + norm_v2) / vnn.max() * (2.0 - gamma)) / (2.0 + norm_v2)
        if alpha < 1.0:
            beta = (4.0 - (2.0 - gamma) / vnn.max()) / (1.0 + 2.0 / norm_v2) ** 2
        else:
            alpha, beta = 1.0, 0.0
        bsca = 2.0 * alpha**2 - beta
        avec = 2.0 - (bsca + 2.0 * alpha**2) * vnn
        invavnn = vnn / avec
        # ---- moments, natural gradient, update of v and d (:331-378) ----
        p_mu, q_mu = (np.zeros(n), np.zeros(n)) if cmu == 0.0 else (p_mu_dev, q_mu_dev)
        p_one, q_one = (np.zeros(n), np.zeros(n)) if c1 == 0.0 else _moments(vn, norm_v2, pc / dvec)
        p = cmu * p_mu
        q = cmu * q_mu
        if cond:
            p = p + c1 * p_one
            q = q + c1 * q_one
        if cmu + c1 > 0.0:
            ngv, ngd = _natural_gradient(dvec, vn, vnn, norm_v, norm_v2, alpha, avec, bsca, invavnn, p, q)
            step = min(1.0, 0.7 * norm_v / np.sqrt(np.dot(ngv, ngv)), 0.7 * (dvec / np.abs(ngd)).min())
            self.vvec = vvec + step * ngv
            self.dvec = dvec + step * ngd
        self._normalise()
        return None, None  # (no B, D: the stopping rules that read them do not apply)


register("vdcma", minimize)
