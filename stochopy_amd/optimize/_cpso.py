"""PSO / CPSO front end + generation loop for ``backend="hip"``.

Reference: stochopy/optimize/cpso/_cpso.py:12-179 (``minimize``: signature, defaults,
validation, sync rule, seeding), :182-321 (``cpso`` loop: init V=0, pbest=X; per-generation
draw order r1 then r2; return_all; callback; restart after the callback) and
stochopy/optimize/pso/_pso.py:9-122 (PSO = CPSO with competitivity None).  The
per-generation work -- mutation (:324-329), Shrink (cpso/_constraints.py:44-53),
selection_sync and the objective -- is one fused HIP kernel plus the one-workgroup
best/termination kernel; the competitive restart (:405-426) is three small kernels
(csrc/sx_pso.hip).
"""
import ctypes as C
import os

import numpy as np

from .. import _device, _lib, _rng
from . import _common, _runs
from ._helpers import register
from ._population import _PopulationRun

__all__ = ["minimize"]


def minimize(
    fun,
    bounds,
    x0=None,
    args=(),
    maxiter=100,
    popsize=10,
    inertia=0.7298,
    cognitivity=1.49618,
    sociability=1.49618,
    competitivity=1.0,
    seed=None,
    xtol=1.0e-8,
    ftol=1.0e-8,
    constraints=None,
    updating="immediate",
    workers=1,
    backend=None,
    return_all=False,
    verbosity=1.0,
    callback=None,
    rng=None,
    strict_updating=None,
    host_workers=None,
    host_backend=None,
    runs=None,
):
    """Minimize an objective function using Competitive PSO on MI355X.

    Parameters are those of the reference (cpso/_cpso.py:12-33) plus ``rng``
    ("numpy-legacy" default = the reference's stream, or "philox" = in-kernel draws);
    ``backend`` must be ``"hip"``.  ``updating="immediate"`` (the reference's default) runs pso_async
    (cpso/_cpso.py:364-402) as one ordered sweep per generation on one GPU whenever that is possible
    (``workers=1``, a factory objective; same seed, same result as the reference's default call); otherwise the
    run is deferred like with a parallel backend of the reference (cpso/_cpso.py:147-150), with a warning.
    ``updating="deferred"`` is the throughput mode; ``strict_updating=False`` forces it silently.
    ``runs=R`` (R >= 2) performs R independent runs with these settings in ONE kernel launch, one workgroup per run
    (csrc/sx_pso_runs.hip): run r is, bit for bit, the run of ``seed + r`` (``seed`` an integer) or of ``seed[r]``
    (a sequence of R integers) with ``rng="philox", updating="deferred"``; ``x0`` is ``None``, one ``(P, n)`` swarm
    for all runs or ``(R, P, n)``, and is not modified.  The result describes the best run (``np.argmin`` over the runs'
    ``fun``; ``run`` is its index, ``nfev`` the sum over all runs) and carries ``xs``, ``funs``, ``nits``, ``statuses``
    per run.  With ``runs=R``, ``inertia``, ``cognitivity``, ``sociability`` and ``competitivity`` may each be a sequence of R
    values, one per run (a sweep: run r is the single run with element r of each and seed r; a run whose ``competitivity``
    is 0 never restarts); the result then has ``sweep``, a dict from the name of each such option to the ``(R,)`` array
    used.  Needs ``rng="philox"``, a factory objective, one GPU, no callback, no ``return_all``, rows of at most
    ``sx_wide_from()`` elements and a swarm that fits one workgroup's LDS (``sx_pso_runs_lds_bytes``).
    A caller's own objective is served with ``runs=R`` when it is declared row-wise, ``factory.batched(f, rowwise=True)``
    (the value of a row depends on that row only), and no run can restart (``competitivity`` ``None`` or 0, for every
    run): the R swarms then live in device memory (csrc/sx_runs_unfused.hip; no LDS limit, ``popsize * R < 2**31``) and
    ``f(X, *args)`` is called ONCE per generation on the stacked ``(R * P, n)`` float64 tensor -- row ``r * P + i`` is
    particle i of run r -- returning ``(R * P,)``.  Run r is, bit for bit, the run ``minimize(factory.batched(f), ...)``
    performs with seed r, ``rng="philox", updating="deferred"``; the other limits and the result are those above.  A run
    that has ended is frozen; ``f`` still receives its last rows until every run has ended.  An undeclared
    ``factory.batched(f)`` is refused with ``runs``.
    """
    batched_runs = _runs.batched(runs)
    fun_id = _common.resolve_objective(fun, args, workers, backend, host_workers, host_backend)
    lower, upper = _common.as_bounds(bounds)
    if batched_runs and x0 is not None and np.ndim(x0) == 3:  # a swarm per run
        if np.shape(x0) != (runs, popsize, len(bounds)):
            raise ValueError(f"x0 of shape {np.shape(x0)} with runs={runs}: expected ({popsize}, {len(bounds)}) for all runs "
                             f"or ({runs}, {popsize}, {len(bounds)})")
    elif x0 is not None:
        if np.ndim(x0) != 2 or np.shape(x0)[1] != len(bounds):
            raise ValueError()
    if popsize < 2:
        raise ValueError()
    if x0 is not None and np.ndim(x0) == 2 and len(x0) != popsize:
        raise ValueError()
    inertia = _runs.per_run("inertia", inertia, runs, 0.0, 1.0)
    cognitivity = _runs.per_run("cognitivity", cognitivity, runs, 0.0, 4.0)
    sociability = _runs.per_run("sociability", sociability, runs, 0.0, 4.0)
    if competitivity is not None:
        competitivity = _runs.per_run("competitivity", competitivity, runs, 0.0, 2.0)
    if updating not in {"immediate", "deferred"}:
        raise ValueError()
    if constraints not in (None, "Shrink"):
        raise KeyError(constraints)
    if callback is not None and not hasattr(callback, "__call__"):
        raise ValueError()
    _common.resolve_backend(backend, fun_id)
    rng = _common.resolve_rng(rng)
    if batched_runs:
        return _minimize_runs(int(runs), fun_id, lower, upper, x0, int(maxiter), int(popsize), _runs.setting(inertia),
                              _runs.setting(cognitivity), _runs.setting(sociability), competitivity, constraints,
                              float(xtol), float(ftol), seed, rng, updating, strict_updating, workers, return_all, callback)
    workers = _common.resolve_workers(workers, fun_id)
    run = _PsoRun(fun_id, lower, upper, x0, int(maxiter), int(popsize), float(inertia), float(cognitivity),
                  float(sociability), competitivity, constraints, float(xtol), float(ftol), bool(return_all),
                  float(verbosity), callback, rng, seed, workers,
                  immediate=_common.resolve_updating(updating, strict_updating, workers, fun_id, len(lower)))
    return run.result()


def _minimize_runs(R, fun_id, lower, upper, x0, maxiter, P, w, c1, c2, competitivity, constraints, xtol, ftol, seed, rng,
                   updating, strict_updating, workers, return_all, callback):
    """``runs=R``: R independent deferred-updating runs, one workgroup each, one launch (csrc/sx_pso_runs.hip).  Everything
    that can be refused is refused before the device is touched."""
    n = len(lower)
    _runs.refuse_common(rng, fun_id, workers, callback, return_all, serves_rowwise=True)
    if _runs.rowwise(fun_id) and competitivity is not None and np.any(competitivity):
        raise ValueError(f"runs > 1 around a factory.batched(f, rowwise=True) objective serves PSO, i.e. competitivity None "
                         f"or 0 for every run (competitivity={competitivity!r}): the competitive restart is not part of "
                         "that path")
    _runs.refuse_immediate(updating, strict_updating, "cpso/_cpso.py:147-150")
    seeds = _runs.seeds_of(R, seed)
    if n > _lib.wide_from():
        raise ValueError(f"runs > 1 serves rows of up to {_lib.wide_from()} elements (n = {n})")
    if _runs.rowwise(fun_id):  # the caller's own objective: the swarms live in device memory, no LDS limit
        if R * P >= 1 << 31:
            raise ValueError(f"runs={R} x popsize {P}: the objective is handed all runs' rows at once, fewer than 2^31")
        batch = _rowwise_batch(seeds, fun_id, lower, upper, x0, maxiter, P, w, c1, c2, constraints, xtol, ftol)
        batch.launch()
        return _runs.result(batch.fetch(), P, inertia=w, cognitivity=c1, sociability=c2, competitivity=competitivity)
    if int(_lib.lib().sx_pso_runs_lds_bytes(P, n)) < 0:
        raise ValueError(f"runs > 1 keeps a run's swarm (X and pbest at the least) in one workgroup's LDS: popsize {P} x {n} "
                         "variables is more than its 160 KiB hold")
    batch = _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, w, c1, c2, competitivity, constraints, xtol, ftol)
    batch.launch()
    return _runs.result(batch.fetch(), P, inertia=w, cognitivity=c1, sociability=c2, competitivity=competitivity)


def _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, w, c1, c2, competitivity, constraints, xtol, ftol, outputs=()):
    """The batch of one sx_pso_runs_launch; ``outputs``: of the optional ones, every run's last swarm -- ``"xfinal"``,
    ``"pbest_final"``, ``"pbestfit_final"``.  ``w``, ``c1``, ``c2``, ``competitivity``: a float or an (R,) array (run r uses
    element r)."""
    n = len(lower)
    if _runs.is_swept(competitivity):
        gamma = competitivity
    else:
        gamma = float(competitivity) if competitivity else 0.0
    # cpso/_cpso.py:215-216 (depends on maxiter and the swarm's size; read by the runs whose gamma is not 0)
    delta = float(np.log(1.0 + 0.003 * P) / np.max((0.2, np.log(0.01 * maxiter)))) if np.any(gamma) else 0.0
    batch = _runs.Batch("sx_pso_runs_launch", _lib.SxPsoRunsArgs(), seeds, P)
    a, ctx, R = batch.a, batch.ctx, batch.R
    with batch.stream():
        batch.upload_keys()
        d_bounds = ctx.upload_async(np.concatenate([lower, upper]))
        batch.bind(lower=d_bounds[:n], upper=d_bounds[n:])
        if x0 is not None:
            batch.bind(x0=ctx.upload(np.array(x0, dtype=np.float64)))
            a.x0_stride = P * n if batch.dev["x0"].dim() == 3 else 0
        batch.outputs(n, {"xfinal": ((R, P, n), None), "pbest_final": ((R, P, n), None), "pbestfit_final": ((R, P), None)},
                      outputs)
        # (a swarm whose X, V and pbest do not fit the LDS together keeps its velocities here)
        vwork = int(ctx.L.sx_pso_runs_workspace_bytes(R, P, n))
        if vwork:
            batch.bind(vwork=ctx.empty((vwork // 8,)))
        own = batch.bind_sweep(w=w, c1=c1, c2=c2, gamma=gamma)
    a.n, a.fun_id = n, fun_id
    a.constraints, a.maxiter = (1 if constraints == "Shrink" else 0), maxiter
    a.w, a.c1, a.c2, a.gamma, a.delta, a.xtol, a.ftol = own["w"], own["c1"], own["c2"], own["gamma"], delta, xtol, ftol
    return batch


def _rowwise_batch(seeds, external, lower, upper, x0, maxiter, P, w, c1, c2, constraints, xtol, ftol):
    """The device-memory batch around a caller's row-wise objective (csrc/sx_runs_unfused.hip): PSO's struct fields and sweep
    arrays.  pop0 is X -- the rows the objective is handed --, pop1 V and pop2 pbest.  ``w``, ``c1``, ``c2``: as in
    ``_runs_batch``."""
    batch = _runs.RowwiseBatch("sx_runs_rowwise_pso_move", external, seeds, lower, upper, x0, maxiter, P,
                               constraints == "Shrink", xtol, ftol)
    with batch.stream():
        own = batch.bind_sweep(w=w, c1=c1, c2=c2)
    batch.a.w, batch.a.c1, batch.a.c2 = own["w"], own["c1"], own["c2"]
    return batch


class _PsoRun(_PopulationRun):
    MEMBERS, WHOLE = "particles", "swarm"
    CHECK_EVERY = 32  # philox mode: the host reads the device state every this many generations
    GRAPH_CHUNK = 16  # generations per hipGraph replay (2 or 5 kernel nodes each)

    def __init__(self, fun_id, lower, upper, x0, maxiter, P, w, c1, c2, gamma, constraints, xtol, ftol, return_all,
                 verbosity, callback, rng, seed, workers, autorun=True, immediate=False):
        super().__init__("cpso" if gamma else "pso", fun_id, lower, upper, x0, maxiter, P, xtol, ftol, return_all, verbosity,
                         callback, rng, seed, workers, immediate)
        self.w, self.c1, self.c2, self.gamma, self.constraints = w, c1, c2, gamma, constraints
        # pso_async assigns X[i] row by row, i.e. works in place on the caller's x0 (cpso/_cpso.py:389)
        self.x0_in_place = immediate
        if self.world is not None and gamma and P % self.world.size != 0:
            # (PSO takes any popsize -- blocks of ceil(P / workers) rows, the last rank short; the competitive restart's
            # swarm-wide selection gathers equal [pbestfit | radii] segments per rank)
            raise ValueError(f"cpso with workers={self.world.size}: popsize={P} must be a multiple of workers (pso, de, "
                             "cmaes and vdcma take any popsize)")
        self.ctx = _device.Context()
        # sharded swarm: the per-generation best travels by peer writes over xGMI (one one-workgroup kernel,
        # parallel.PeerExchange) when that transport passes its self-test on every rank, else by one all-gather
        self.px, self.exchange, self.exchange_note = self._negotiate_exchange()
        if autorun:
            self._autorun()

    # ------------------------------------------------------------------ setup
    def _setup(self):
        ctx, P, n = self.ctx, self.P, self.n
        t = _device.torch()
        self.stream = _rng.make_init_stream(self.rng, self.seed)
        if self.gamma:  # cpso/_cpso.py:215-216 (depends on maxiter; the whole swarm's size)
            self.delta = np.log(1.0 + 0.003 * self.Ptotal) / np.max((0.2, np.log(0.01 * self.maxiter)))
        self.d_lower = ctx.upload(self.lower)
        self.d_upper = ctx.upload(self.upper)
        if self.x0 is None and self.rng == "philox":
            # in-kernel draws: the Latin hypercube is drawn on the device too, every rank its own rows (_rng.py)
            self.X = _rng.philox_latin_hypercube(ctx, ctx.empty((P, n)), self.row0, self.Ptotal, self.d_lower,
                                                 self.d_upper, self.seed)
        else:
            if self.x0 is not None:
                X0 = np.array(self.x0, dtype=np.float64)
            else:
                X0 = self.stream.latin_hypercube(self.Ptotal, n, self.lower, self.upper)
            if self.world is not None:
                X0 = np.ascontiguousarray(X0[self.row0 : self.row0 + P])
            self.X = ctx.upload(X0)
        self.V = ctx.zeros((P, n))
        self.pbest = self.X.clone()
        npart = int(ctx.L.sx_num_partials(P, n))
        self.npart = npart
        # [pbestfit | partial radii] in one buffer: with workers > 1 the restart all-gathers exactly this
        self.fit_radius = ctx.empty((P + npart,))
        self.pbestfit = self.fit_radius[:P]
        self.part_r = self.fit_radius[P:]
        if self.world is not None and self.gamma:
            self.fit_radius_all = ctx.empty((self.world.size, P + npart))
        self.candfit = ctx.empty((P,))
        self.part_f = ctx.empty((npart,))
        self.part_i = ctx.empty((npart,), dtype=t.int64)
        self.sel3 = ctx.zeros((3,), dtype=t.int64)
        _common.evaluate_rows(ctx, self.fun_id, self.X, n, self.pbestfit)
        self.candfit.copy_(self.pbestfit)
        out_i = ctx.empty((1,), dtype=t.int64)
        out_f = ctx.empty((1,))
        _lib.check(ctx.L.sx_argmin(_device.ptr(self.pbestfit), P, _device.ptr(self.part_f), _device.ptr(self.part_i),
                                   npart, _device.ptr(out_i), _device.ptr(out_f), ctx.stream_ptr), "sx_argmin")
        g = int(out_i.cpu()[0])
        gfit0 = float(out_f.cpu()[0])
        self.gbest = self.X[g].clone()
        if self.world is not None:  # initial global best: one record exchange, settled on the host
            from ..parallel import best_of_records

            self.record = ctx.empty((n + 2,))
            self.records = ctx.empty((self.world.size, n + 2))
            self.record[0] = gfit0
            self.record[1] = float(self.row0 + g)
            self.record[2:].copy_(self.gbest)
            self.world.all_gather_records(self.record, self.records)
            wbest, gfit0, g = best_of_records(self.records.cpu().numpy())
            self.gbest.copy_(self.records[wbest, 2:])
        st = _lib.SxState(it=1, gbidx=g, gfit=gfit0, dx=0.0, status=_lib.SX_STATUS_NONE, done=0)
        self.state = ctx.upload(np.frombuffer(bytes(st), dtype=np.int64).copy())
        key0, key1 = _rng.philox_key(self.seed) if self.rng == "philox" else (0, 0)
        a = _lib.SxPsoArgs()
        a.X, a.V, a.pbest = self.X.data_ptr(), self.V.data_ptr(), self.pbest.data_ptr()
        a.pbestfit, a.candfit, a.gbest = self.pbestfit.data_ptr(), self.candfit.data_ptr(), self.gbest.data_ptr()
        a.lower, a.upper, a.state = self.d_lower.data_ptr(), self.d_upper.data_ptr(), self.state.data_ptr()
        a.part_f, a.part_i = self.part_f.data_ptr(), self.part_i.data_ptr()
        a.P, a.ld, a.row0, a.n = P, n, self.row0, n
        a.fun_id = self.fun_id if self.external is None else 0
        if self.external is not None:
            self.cand_f = ctx.empty((P,))
        a.constraints = 1 if self.constraints == "Shrink" else 0
        a.rng = _lib.SX_RNG_PHILOX if self.rng == "philox" else _lib.SX_RNG_HOST
        a.maxiter = self.maxiter
        a.w, a.c1, a.c2, a.xtol, a.ftol = self.w, self.c1, self.c2, self.xtol, self.ftol
        a.key0, a.key1 = key0, key1
        self.args = a
        if self.rng == "numpy-legacy":
            self.h_r = [t.empty((P, n), dtype=t.float64).pin_memory() for _ in range(2)]
            self.d_r = [ctx.empty((P, n)) for _ in range(2)]
            a.r1, a.r2 = self.d_r[0].data_ptr(), self.d_r[1].data_ptr()
        if self.world is not None and (self.return_all or self.callback is not None):
            self.Xfull = ctx.empty((self.Ptotal, n))
            self.candfull = ctx.empty((self.Ptotal,))
        if self.return_all:
            self.nout = int(np.ceil(self.verbosity * self.Ptotal))
            rows = max(self.nout, 1)
            self.xall = ctx.empty((self.maxiter, rows, n))
            self.funall = ctx.empty((self.maxiter, rows))
            if self.nout > 0:
                X1, f1 = self._whole_population(1)  # candfit == pbestfit for the initial swarm
                self.xall[0].copy_(X1[: self.nout])
                self.funall[0].copy_(f1[: self.nout])
            else:
                self.xall[0, 0].copy_(self.gbest)
                self.funall[0, 0] = st.gfit
        self.st = st
        self.restarts = []

    # --------------------------------------------------------------- helpers
    def _population(self, it):
        return self.X

    def _best_row(self, st):
        """The swarm's best position (host copy)."""
        return self.gbest.cpu().numpy()

    def _settle_status(self, st):
        return int(st.status)

    def _generation(self):
        ctx = self.ctx
        if self.rng == "numpy-legacy":  # cpso/_cpso.py:262-263: r1 then r2
            for h, d in zip(self.h_r, self.d_r):
                self.stream.random(None, out=h.numpy())
                d.copy_(h, non_blocking=True)
        if self.immediate:
            _lib.check(ctx.L.sx_pso_async_generation(C.byref(self.args), ctx.stream_ptr), "sx_pso_async_generation")
            return
        p, n = _device.ptr, self.n
        if self.external is not None:
            # around the caller's objective (csrc/sx_unfused.hip): move, evaluate the new positions, pbest selection
            _lib.check(ctx.L.sx_pso_move(C.byref(self.args), ctx.stream_ptr), "sx_pso_move")
            self.cand_f.copy_(self.external(ctx, self.X))
            _lib.check(ctx.L.sx_rows_select(p(self.X), n, p(self.cand_f), p(self.pbest), p(self.pbest), n,
                                            p(self.pbestfit), p(self.candfit), self.P, n, p(self.state),
                                            p(self.part_f), p(self.part_i), ctx.stream_ptr), "sx_rows_select")
            if self.world is None:
                _lib.check(ctx.L.sx_select_finalize(p(self.part_f), p(self.part_i), self.npart, p(self.pbest),
                                                    p(self.pbest), n, n, p(self.gbest), p(self.state), self.maxiter,
                                                    self.xtol, self.ftol, ctx.stream_ptr), "sx_select_finalize")
                return
        elif self.world is None:
            _lib.check(ctx.L.sx_pso_generation(C.byref(self.args), 1, ctx.stream_ptr), "sx_pso_generation")
            return
        else:  # sharded swarm: local generation, then the global-best exchange (parallel.py)
            _lib.check(ctx.L.sx_pso_generation(C.byref(self.args), 0, ctx.stream_ptr), "sx_pso_generation")
        if self.px is not None:
            _lib.check(ctx.L.sx_xchg_finalize(p(self.part_f), p(self.part_i), self.npart, p(self.pbest), p(self.pbest),
                                              n, n, self.row0, p(self.gbest), p(self.state), self.maxiter, self.xtol,
                                              self.ftol, C.byref(self.px.args), ctx.stream_ptr), "sx_xchg_finalize")
            return
        _lib.check(ctx.L.sx_shard_best(p(self.part_f), p(self.part_i), self.npart, p(self.pbest), p(self.pbest), n, n,
                                       p(self.state), self.row0, p(self.record), ctx.stream_ptr), "sx_shard_best")
        self.world.all_gather_records(self.record, self.records)
        _lib.check(ctx.L.sx_gather_finalize(p(self.records), self.world.size, n, p(self.gbest), p(self.state),
                                            self.maxiter, self.xtol, self.ftol, ctx.stream_ptr), "sx_gather_finalize")

    def _restart_device(self):
        """cpso/_cpso.py:405-426 entirely on the device (Philox positions keyed by row)."""
        ctx, a = self.ctx, C.byref(self.args)
        _lib.check(ctx.L.sx_pso_radius(a, _device.ptr(self.part_r), ctx.stream_ptr), "sx_pso_radius")
        if self.world is None:
            _lib.check(ctx.L.sx_pso_restart_select(a, _device.ptr(self.part_r), float(self.delta), float(self.gamma),
                                                   _device.ptr(self.sel3), ctx.stream_ptr), "sx_pso_restart_select")
        else:
            # the swarm radius is a max and the worst-nw rule a rank over ALL particles: one all-gather of
            # [pbestfit | partial radii] per generation, then every rank derives the same threshold
            self.world.all_gather_records(self.fit_radius, self.fit_radius_all)
            _lib.check(ctx.L.sx_pso_restart_select_gathered(a, _device.ptr(self.fit_radius_all), self.world.size,
                                                            float(self.delta), float(self.gamma),
                                                            _device.ptr(self.sel3), ctx.stream_ptr),
                       "sx_pso_restart_select_gathered")
        _lib.check(ctx.L.sx_pso_restart_apply(a, _device.ptr(self.sel3), None, None, 0, ctx.stream_ptr),
                   "sx_pso_restart_apply")

    def _restart_host_order(self, it):
        """numpy-legacy stream: the new positions are drawn on the host for the rows in the reference's
        descending-fitness order (cpso/_cpso.py:420-422), so row selection happens on the host too."""
        ctx, P, n = self.ctx, self.P, self.n
        _lib.check(ctx.L.sx_pso_radius(C.byref(self.args), _device.ptr(self.part_r), ctx.stream_ptr), "sx_pso_radius")
        radius = float(self.part_r.max().cpu()) / np.sqrt(4.0 * n)
        if not radius < self.delta:
            return
        inorm = it / self.maxiter
        nw = int((P - 1.0) / (1.0 + np.exp(1.0 / 0.09 * (inorm - self.gamma + 0.5))))
        if nw <= 0:
            return
        rows = self.pbestfit.cpu().numpy().argsort()[: -nw - 1 : -1]
        newx = self.stream.uniform_rows(self.lower, self.upper, nw)
        d_rows = ctx.upload(np.ascontiguousarray(rows, dtype=np.int64))
        d_newx = ctx.upload(newx)
        _lib.check(ctx.L.sx_pso_restart_apply(C.byref(self.args), None, _device.ptr(d_rows), _device.ptr(d_newx), nw,
                                              ctx.stream_ptr), "sx_pso_restart_apply")
        ctx.sync()  # d_rows / d_newx must outlive the kernel
        self.restarts.append((it, nw))

    def _after_generation(self, it):
        """The competitive restart (cpso/_cpso.py:296-300, after the callback)."""
        if self.gamma:
            if self.rng == "numpy-legacy":
                self._restart_host_order(it)
            else:
                self._restart_device()

    # ------------------------------------------------------------------ loop
    def _enqueue_external(self, remaining):
        """A caller's device objective between our kernels: chunks of generations captured into one graph (kernels +
        objective) and replayed, else eagerly."""
        todo = min(remaining, self.CHECK_EVERY)
        while todo >= self.GRAPH_CHUNK and self._capture_sharded_chunk():
            self._rccl_graph.replay()
            todo -= self.GRAPH_CHUNK
        for _ in range(todo):
            self._generation()
            if self.gamma:
                self._restart_device()

    def _enqueue_and_look(self, st, remaining):
        self.enqueue(min(remaining, self.CHECK_EVERY))
        return self.read_state()

    def enqueue(self, ngen):
        """Enqueue `ngen` generations (and their restarts) without host synchronisation (Philox mode).
        Single GPU: full chunks replay one instantiated hipGraph of the loop body."""
        ctx = self.ctx
        if self.world is None:
            while ngen >= self.GRAPH_CHUNK:
                if self._graph is None:
                    g = C.c_void_p()
                    restart = bool(self.gamma)
                    _lib.check(ctx.L.sx_pso_graph_create(
                        C.byref(self.args), self.GRAPH_CHUNK, _device.ptr(self.part_r) if restart else None,
                        float(self.delta) if restart else 0.0, float(self.gamma) if restart else 0.0,
                        _device.ptr(self.sel3) if restart else None, C.byref(g)), "sx_pso_graph_create")
                    self._graph = g
                _lib.check(ctx.L.sx_graph_launch(self._graph, ctx.stream_ptr), "sx_graph_launch")
                ngen -= self.GRAPH_CHUNK
        elif self.world is not None:
            # sharded swarm: kernels + the RCCL all-gathers of a chunk of generations captured once and replayed
            while ngen >= self.GRAPH_CHUNK and self._capture_sharded_chunk():
                self._rccl_graph.replay()
                ngen -= self.GRAPH_CHUNK
        for _ in range(ngen):
            self._generation()
            if self.gamma:
                self._restart_device()

    def _capture_sharded_chunk(self):
        """GRAPH_CHUNK sharded generations (kernels + all-gathers) as one graph; False if that is not possible
        (gloo stages through the host; SX_RCCL_GRAPH=0; a failed capture) -- same collectives either way."""
        if self._rccl_graph is not None:
            return True
        if (self._rccl_graph_note is not None or (self.world is not None and self.world.backend != "nccl")
                or os.environ.get("SX_RCCL_GRAPH") == "0"
                or (self.external is not None and (os.environ.get("SX_EXT_GRAPH") == "0"
                                                   or not getattr(self.external, "capturable", True)))):
            return False
        self._rccl_graph = self._capture(self.GRAPH_CHUNK, self._generation_and_restart, "_rccl_graph_note")
        return self._rccl_graph is not None

    def _generation_and_restart(self):
        self._generation()
        if self.gamma:
            self._restart_device()


register("cpso", minimize)
