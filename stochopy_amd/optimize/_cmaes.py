"""CMA-ES front end + model for ``backend="hip"``; the generation loops are the shared ones of _evolution.py.

Reference: stochopy/optimize/cmaes/_cmaes.py:12-140 (``minimize``) and :143-357 (``cmaes``
loop), :360-434 (``converge``).  On the device (csrc/sx_cmaes.hip, csrc/sx_core.hip):
sampling ``arx = xmean + sigma*B*(D o z)`` and the covariance update as fp64 MFMA
contractions, the objective (fused un-standardisation), the recombination of the
mean.  On the host, as in the reference: ranking (``np.argsort``), the evolution paths,
the step size, the ten stopping rules and -- SURVEY.md section 8f rank 1, "next" -- the
eigendecomposition (``numpy.linalg.eigh`` = LAPACK, the reference's own third-party call),
which also fixes the eigenvector signs the same-seed parity depends on.
``constraints="Penalize"`` (cmaes/_constraints.py:4-82): the clipping of the
candidates, the objective and the weighted squared excess run in one device kernel
(``sx_cmaes_eval_penalized``); the scalar bookkeeping of the boundary weights stays on the host.
"""

import os
import warnings

import numpy as np

from .. import _device, _lib
from ..linalg import Eigh
from . import _common, _evolution, _runs
from ._helpers import register

__all__ = ["minimize"]

_SHORT_OF_TOLERANCE = ("stochopy_amd: the device eigensolver did not reach its tolerance in 60 sweeps; the decomposition is "
                       "used as it is")
_OUT_OF_SWEEPS = ("stochopy_amd: a warm-started decomposition ran out of its %d launched sweeps short of the tolerance (its "
                  "result is used as it is); later ones get the full allowance")


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
    eigh=None,
    host_workers=None,
    host_backend=None,
    runs=None,
):
    """Minimize an objective function using CMA-ES on MI355X (reference cmaes/_cmaes.py:12-30).

    ``eigh="host"`` decomposes C with numpy/LAPACK exactly like the reference (cmaes/_cmaes.py:304 -- the
    reference's own third-party call), whose eigenvector SIGNS (an accident of LAPACK's internals) same-seed
    parity with the reference depends on: the default in the parity mode ``rng="numpy-legacy"``.
    ``eigh="device"`` keeps C on the GPU and decomposes it with this package's own eigensolver
    (csrc/sx_eigh.hip: parallel block Jacobi on the fp64 matrix cores): same
    eigenvalues and eigenvectors to rounding, signs by a stated rule (largest component positive), no
    2 x n^2 PCIe trip -- the default in the throughput mode ``rng="philox"``; the oracle reproduces such runs
    with ``eigh="canonical"`` (LAPACK + the same sign rule).
    ``eigh=callable``: ``callable(C) -> (eigenvalues, eigenvectors)`` replaces the host decomposition (another solver,
    or -- tests/test_gpu_cmaes.py -- the reference's own eigenpairs replayed, which makes same-seed parity checkable
    for shapes whose covariance has a repeated eigenvalue, where no two solvers agree on a basis).

    ``workers > 1`` (one process per GPU) shards what the reference's parallel backends shard -- the
    candidates: every rank samples and evaluates ``popsize / workers`` rows (same draws: the legacy stream is
    replicated on the hosts, Philox normals are keyed by the global row), one all-gather per generation
    returns all candidates and fitness values to every rank, and the O(n^2)/O(n^3) model update is replicated.
    Same result as ``workers=1`` on every rank.

    ``runs=R`` (R >= 2) performs R independent runs with these settings in ONE kernel launch, one workgroup per run
    (csrc/sx_cma_runs.hip): run r is the run of ``seed + r`` (``seed`` an integer) or of ``seed[r]`` (a sequence of R
    integers) with ``rng="philox"`` -- the same draws, the same arithmetic up to the order of its sums; ``x0`` is ``None``
    (every run draws its initial mean as the single run of its seed does), one ``(n,)`` point for all runs or ``(R, n)``.
    The result describes the best run (``np.argmin`` over the runs' ``fun``; ``run`` is its index, ``nfev`` the sum over all
    runs) and carries ``xs``, ``funs``, ``nits``, ``statuses`` and ``sigmas`` (the final step sizes) per run.  With
    ``runs=R``, ``sigma`` may be a sequence of R values, one per run (a sweep: run r starts from ``sigma[r]``, which is
    also what its stopping rules -6 and -8 compare with, as in the single run); the result then has ``sweep``, the dict
    ``{"sigma": the (R,) array used}``.  Needs
    ``rng="philox"``, a factory objective, one GPU, no callback, no ``return_all``, ``constraints=None``, the device
    eigensolver, ``ndim <= 32`` and a population that fits one workgroup's LDS (``sx_cma_runs_lds_bytes``).
    """
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
                              float(muperc), float(xtol), float(ftol), seed, rng, constraints, eigh, workers, return_all,
                              callback)
    workers = _common.resolve_workers(workers, fun_id)
    if len(lower) > _lib.NARROW_DIM:
        # the one method that keeps a dimension cap: an n x n covariance, its eigenvectors and an O(n^3) decomposition per
        # update (cmaes/_cmaes.py:290-309).  Every other method serves rows of up to _lib.WIDE_DIM elements.
        raise ValueError(f"method='cmaes' keeps the full {len(lower)} x {len(lower)} covariance and its eigendecomposition on "
                         f"the device: ndim <= {_lib.NARROW_DIM}.  method='vdcma' is the O(n) variant for long vectors.")
    if eigh is None:
        eigh = "host" if rng == "numpy-legacy" else "device"
    if not callable(eigh) and eigh not in ("host", "device"):
        raise ValueError("eigh must be 'host', 'device' or a callable C -> (eigenvalues, eigenvectors)")
    if eigh == "device" and _evolution.device_loop_serves(fun_id, rng, len(lower), popsize, constraints):
        # the whole loop (and the history) stays on the device -- since round 3 including constraints="Penalize" (its
        # boundary-weight bookkeeping: cma_penalty_kernel), workers > 1 (every rank samples and evaluates its share of the
        # candidates, one all-gather, replicated model) and a callback (the host then looks at every generation and copies
        # what the callback is shown).  SX_CMA_LOOP=host: the host-driven loop with the device eigensolver.
        return _CmaDeviceRun(fun_id, lower, upper, x0, int(maxiter), int(popsize), float(sigma), float(muperc),
                             float(xtol), float(ftol), seed, bool(return_all), float(verbosity),
                             penalize=constraints == "Penalize", workers=workers, callback=callback).run()
    return _CmaRun(fun_id, lower, upper, x0, int(maxiter), int(popsize), float(sigma), float(muperc), float(xtol),
                   float(ftol), bool(return_all), float(verbosity), callback, rng, seed, eigh=eigh, workers=workers,
                   penalize=constraints == "Penalize").run()


def _strategy_constants(n, P, muperc):
    """cmaes/_cmaes.py:184-205."""
    mu, w, mueff, cc = _evolution.selection_weights(n, P, muperc)
    cs = (mueff + 2.0) / (n + mueff + 5.0)
    c1 = 2.0 / ((n + 1.3) ** 2 + mueff)
    cmu = min(1.0 - c1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((n + 2.0) ** 2 + mueff))
    damps = 1.0 + 2.0 * max(0.0, np.sqrt((mueff - 1.0) / (n + 1.0)) - 1.0) + cs
    chind = np.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n**2))
    return mu, w, mueff, cc, cs, c1, cmu, damps, chind


RUNS_MAX_DIM = 32  # runs > 1: the range of the one-workgroup eigensolver (csrc/sx_eigh.hip kSmallPathMax)


def _minimize_runs(R, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, seed, rng, constraints, eigh, workers,
                   return_all, callback):
    """``runs=R``: R independent runs, one workgroup each, one launch (csrc/sx_cma_runs.hip).  Everything that can be
    refused is refused before the device is touched."""
    n = len(lower)
    _runs.refuse_common(rng, fun_id, workers, callback, return_all)
    _runs.refuse_constraints(constraints)
    if eigh is not None and (callable(eigh) or eigh != "device"):
        raise ValueError('runs > 1 decomposes C inside the run\'s kernel: eigh=None or "device" '
                         f"(eigh={'a callable' if callable(eigh) else repr(eigh)})")
    seeds = _runs.seeds_of(R, seed)
    _runs.refuse_maxiter(maxiter)
    if n > RUNS_MAX_DIM:
        raise ValueError(f"runs > 1 keeps a run's covariance and its eigendecomposition in one workgroup: ndim <= "
                         f"{RUNS_MAX_DIM} (ndim = {n}, popsize = {P})")
    lds = int(_lib.lib().sx_cma_runs_lds_bytes(P, n)) if P >= 1 else -1
    mu = int(muperc * P)
    if lds < 0 or mu < 1:
        raise ValueError(f"runs > 1 keeps a run's model and candidates in one workgroup's LDS: popsize {P} x {n} variables "
                         f"(mu = {mu}) needs 2 <= popsize, mu >= 1 and at most 160 KiB")
    batch = _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol)
    batch.launch()
    return _runs.result(batch.fetch(), P, sigma=sigma)


def _runs_batch(seeds, fun_id, lower, upper, x0, maxiter, P, sigma, muperc, xtol, ftol, outputs=()):
    """The batch of one sx_cma_runs_launch; ``outputs``: of the optional ones, ``"nfevs"`` and ``"xmeans"`` (every run's
    final mean, standardised).  ``sigma``: a float or an (R,) array (run r starts from element r)."""
    n, R = len(lower), len(seeds)
    mu, w, *constants = _strategy_constants(n, P, muperc)
    xm, xstd, xmean0 = _runs.standardised(lower, upper, x0, R)
    if xmean0 is None:
        # the initial mean of the single run of each seed: its private legacy stream (_rng.make_init_stream), n uniforms
        xmean0 = np.array([np.random.RandomState(s & 0xFFFFFFFF).uniform(-1.0, 1.0, n) for s in seeds])
    batch = _runs.Batch("sx_cma_runs_launch", _lib.SxCmaRunsArgs(), seeds, P)
    a, ctx = batch.a, batch.ctx
    with batch.stream():
        batch.upload_keys()
        d_xmean0, d_std, d_w = ctx.upload(xmean0), ctx.upload_async(np.concatenate([xm, xstd])), ctx.upload(w)
        batch.bind(xmean0=d_xmean0, xm=d_std[:n], xstd=d_std[n:], w=d_w,
                   work=ctx.empty((int(ctx.L.sx_cma_runs_workspace_bytes(R, maxiter)) // 8,)))
        batch.outputs(n, {"nfevs": ((R,), _device.torch().int64), "xmeans": ((R, n), None)}, outputs, extra=("sigmas",))
        own = batch.bind_sweep(sigma=sigma)
    _runs.set_model_scalars(a, n, mu, fun_id, maxiter, own["sigma"], xtol, ftol)
    a.mueff, a.cc, a.cs, a.c1, a.cmu, a.damps, a.chind = constants
    return batch


COLD_SWEEPS = 40   # launched for a decomposition started from the identity (n=512: 11-13 are carried out)
WARM_SWEEPS0 = 16  # launched for the first warm-started one; afterwards: what the last one needed + 1


def decomposition_due(gen, eigeneval, P, c1, cmu, n):
    """Does generation ``gen`` decompose C (cmaes/_cmaes.py:301), ``eigeneval`` being ``gen * P`` of the last one that did (0:
    none yet)?  0: no; 1: the first, started from the identity; 2: started from the previous eigenvectors (C changes by
    O(c1 + cmu) between two)."""
    if gen * P - eigeneval > P / (c1 + cmu) / n / 10.0:
        return 2 if eigeneval else 1
    return 0


def look_cap(n, most):
    """Generations between two looks of the device-resident loop (about 2 ms of them; reached by doubling).  A function of
    the problem, not of the clock or of the number of ranks: the sweep allowance follows what the host has SEEN."""
    return 1 if n > 256 else min(most, max(1, 512 // max(n, 32)))


def sweep_allowance(used, ok, fails, fails_seen, launched, look_cap, warned_short):
    """What a look at the eigensolver's record (the last decomposition used ``used`` of the ``launched`` sweeps and
    converged or not; ``fails`` decompositions since the start fell short, ``fails_seen`` of them known) allows the next
    warm-started decomposition: (sweeps to launch, fails_seen, warning or None).  Launches beyond convergence are no-ops of
    ~2 us each, 2n/16 - 1 per sweep; inside a run the count moves by at most one between decompositions
    (tools/eigh_c4_sweeps.py), and the record is the LAST decomposition's: between rarer looks it gets two more sweeps
    of slack."""
    if ok and fails == fails_seen:
        return min(60, used + (1 if look_cap == 1 else 3)), fails_seen, None
    if launched >= 60:
        return 60, fails, _SHORT_OF_TOLERANCE
    return 60, fails, None if warned_short else _OUT_OF_SWEEPS % launched


class _CmaDeviceRun(_evolution._DeviceRun):
    """The reference's loop (cmaes/_cmaes.py:226-343) with every per-generation step on the device
    (csrc/sx_cma_loop.hip): the host only works out, from the generation number, when the eigendecomposition is due
    (:301) and how many sweeps to launch for it.  Eigenvectors with the canonical sign of csrc/sx_eigh.hip."""

    NAME, Args, ENTRY, GATHERED = "CMA-ES", _lib.SxCmaArgs, "sx_cmaes_generation", ("arx", "fit")

    def _model(self, init):
        ctx, n, P = self.ctx, self.n, self.P
        self.mu, self.w, *self.constants = _strategy_constants(n, P, self.muperc)
        self.c1, self.cmu = self.constants[3:5]
        eig = self.eig = Eigh(ctx, n)
        return dict(arx=ctx.empty((P, n)), ps=ctx.zeros((n,)), C=ctx.upload(np.eye(n)), B=ctx.upload(np.eye(n)),
                    D=ctx.upload(np.ones(n)), eigw=eig.w, Y=ctx.empty((self.mu, n)), part=ctx.empty((64, n)),
                    step=ctx.empty((n,)), isc=ctx.empty((n,)), xnew=ctx.empty((n,)), ypart=ctx.empty((8, n)), eigh_ws=eig.ws)

    def _scalar_args(self, a):
        a.mueff, a.cc, a.cs, a.c1, a.cmu, a.damps, a.chind = self.constants
        a.eigh_ws_bytes, a.eig_sweeps = self.eig.bytes, COLD_SWEEPS

    def _look_cap(self):
        return look_cap(self.n, self.LOOK)

    def _begin(self):
        L, n = self.ctx.L, self.n
        self._eigeneval, self._fails_seen, self._warned_short = 0, 0, False
        self._pin_state = self._pin_eig = None
        self._warm_sweeps, self._launched, self._decomposed = WARM_SWEEPS0, 0, False
        # Large n, one GPU, no callback (the host looks at every generation anyway, look cap 1): the decomposition is
        # enqueued in PIECES (_enqueue_phased) instead of a whole sweep of no-op launches "in case" (~30 of 3.5 us per
        # decomposition at n = 512).
        self._rps = rps = int(L.sx_eigh_rounds_per_sweep(n))
        self._phased = (self.world is None and self.callback is None and self._look_cap() == 1 and rps > 0
                        and os.environ.get("SX_CMA_PHASED", "1") != "0")
        self._warm_rounds = None  # rounds the last phased decomposition needed
        self._cap_hit = False     # the last phased decomposition was still open when the round cap was reached

    def _enqueue(self, gen):
        due = decomposition_due(gen, self._eigeneval, self.P, self.c1, self.cmu, self.n)
        if due:
            self._eigeneval = gen * self.P
            self.args.eig_sweeps = self._launched = COLD_SWEEPS if due == 1 else self._warm_sweeps
            self._decomposed = True
            if self._phased:
                return self._enqueue_phased(gen, due)
        self._generation(gen, due)

    def _pins(self):
        t = _device.torch()
        if self._pin_state is None:
            self._pin_state = t.empty_like(self.buffers["state"], device="cpu").pin_memory()
            self._pin_eig = t.empty((256,), dtype=t.float64).pin_memory()
        return self._pin_state, self._pin_eig

    def _enqueue_phased(self, gen, due):
        """A decomposing generation in pieces (sx_cmaes_generation_phased): the rounds the last decomposition needed, one
        look at the solver's run record, then either its finish or another sweep.  That look also returns the state record
        the PREVIOUS generation's stop rules wrote, so the host still waits once per generation (the stop is seen one
        generation late: what was enqueued in between does nothing); returns that record."""
        rps, ctx = self._rps, self.ctx
        pin_state, pin_eig = self._pins()
        cap = 60 * rps
        r1 = min(cap, self._warm_rounds if (due == 2 and self._warm_rounds) else 8 * rps + 2)
        self._call("sx_cmaes_generation_phased", gen, due, 0, 0, r1)
        while True:
            pin_state.copy_(self.buffers["state"], non_blocking=True)
            pin_eig.copy_(self.eig.ws[:256], non_blocking=True)
            ctx.sync()
            state = _lib.SxCmaState.from_buffer_copy(pin_state.numpy().tobytes())  # (of generation gen - 1)
            rec = pin_eig.numpy().view(np.int32)  # EighInfo: done_seq, sweeps, parity, converged, ...
            if state.done or rec[0] != 0 or r1 >= cap:
                break
            r0, r1 = r1, min(cap, r1 + rps)
            self._call("sx_cmaes_generation_phased", gen, due, 1, r0, r1)
        if state.done:
            return state
        # (the look above also shows what the PREVIOUS generation's closing kernel made of a run that had hit the cap)
        fails = int(rec[510])  # (byte 2040) decompositions since the start that fell short of the tolerance
        if fails != self._fails_seen:
            if self._cap_hit:
                warnings.warn(_SHORT_OF_TOLERANCE, RuntimeWarning, stacklevel=5)
            self._fails_seen = fails
        self._cap_hit = False
        self._call("sx_cmaes_generation_phased", gen, due, 2, 0, r1)
        if rec[0] != 0:  # ended within what was enqueued: it carried out rec[1] sweeps and the two rounds that tell
            self._warm_rounds = int(rec[1]) * rps + 2
        else:
            # the round cap was hit with the run still open.  Phase 2's closing kernel may yet accept the result through
            # the refinement criterion (eigh_close_kernel) and counts a short-fall on the device otherwise: the verdict
            # is read from that counter at the next look, not guessed here
            self._cap_hit = True
            self._warm_rounds = None
        self._decomposed = False
        return state

    def _look(self):
        """ONE trip to the device per look: the state record and (when a decomposition was enqueued since the last look)
        the head of the eigensolver's workspace -- its run record and the count of runs that fell short -- through pinned
        memory behind a single synchronisation."""
        pin_state, pin_eig = self._pins()
        pin_state.copy_(self.buffers["state"], non_blocking=True)
        if self._decomposed:
            pin_eig.copy_(self.eig.ws[:256], non_blocking=True)
        self.ctx.sync()
        return _lib.SxCmaState.from_buffer_copy(pin_state.numpy().tobytes())

    def _after_look(self):
        if not self._decomposed:  # (the record is only meaningful once a decomposition has been enqueued)
            return
        rec = self._pin_eig.numpy().view(np.int32)  # csrc/sx_eigh.hip EighInfo: done_seq, sweeps, parity, converged, ...
        self._warm_sweeps, self._fails_seen, warning = sweep_allowance(
            int(rec[1]), bool(rec[3]), int(rec[510]), self._fails_seen, self._launched, self._look_cap(), self._warned_short)
        if warning is not None:
            warnings.warn(warning, RuntimeWarning, stacklevel=4)
            self._warned_short = self._warned_short or self._launched < 60
        self._decomposed = False

    def _last_state(self, state):
        if not state.done:  # (the phased loop sees a generation's record one look late)
            state = self.read_state()
        if self._cap_hit and int(self.eig.ws[:256].cpu().numpy().view(np.int32)[510]) != self._fails_seen:
            warnings.warn(_SHORT_OF_TOLERANCE, RuntimeWarning, stacklevel=4)  # the run's last decomposition
        return state


class _CmaRun(_evolution._HostRun):
    """The host-driven loop: sampling, recombination and the covariance update on the device, paths, step size and (but
    for ``eigh="device"``) the eigendecomposition on the host."""

    def __init__(self, *args, eigh="host", **kwargs):
        self.eigh = eigh
        super().__init__(*args, **kwargs)

    def _setup(self):
        ctx, n, P, t = self.ctx, self.n, self.P, _device.torch()
        self.mu, self.w, self.mueff, *self.constants = _strategy_constants(n, P, self.muperc)
        self.pc, self.ps = np.zeros(n), np.zeros(n)
        self.B, self.D, self.invsqrtC, self.diagC = np.eye(n), np.ones(n), np.eye(n), np.ones(n)
        self.d_w = ctx.upload(self.w)
        self.d_C, self.d_B, self.d_D = ctx.upload(np.eye(n)), ctx.upload(self.B), ctx.upload(self.D)
        self.d_xmean, self.d_xold, self.d_pc = ctx.upload(self.xmean), ctx.empty((n,)), ctx.empty((n,))
        self.d_idx = ctx.empty((self.mu,), dtype=t.int64)
        self.d_Y = ctx.empty((self.mu, n))  # artmp scratch of the covariance update
        self.eigeneval = 0
        self.eig, self.eig_sweeps = None, COLD_SWEEPS  # launches beyond convergence are no-ops, but not free

    def _sample(self, it):
        """arx = xmean + sigma * B (D o z) (device GEMM)."""
        ptr = _device.ptr
        _lib.check(self.ctx.L.sx_cmaes_sample(ptr(self.d_xmean), self.sigma, ptr(self.d_B), ptr(self.d_D), ptr(self.d_Z),
                                              ptr(self.d_arx_loc), self.Pl, self.n, self.ctx.stream_ptr), "sx_cmaes_sample")

    def _update(self, it, arfit, order):
        ctx, L, n, P, mu, ptr, t = self.ctx, self.ctx.L, self.n, self.P, self.mu, _device.ptr, _device.torch()
        sp = ctx.stream_ptr
        cc, cs, c1, cmu, damps, chind = self.constants
        mueff, sigma, B, D = self.mueff, self.sigma, self.B, self.D
        # ---- recombine (cmaes/_cmaes.py:272-277) ----
        self.d_idx.copy_(t.from_numpy(np.ascontiguousarray(order[:mu], dtype=np.int64)), non_blocking=False)
        xold = self.xold = self.xmean
        self.d_xold.copy_(self.d_xmean)
        _lib.check(L.sx_cmaes_recombine(ptr(self.d_arx), ptr(self.d_idx), ptr(self.d_w), mu, n, ptr(self.d_xmean), sp),
                   "sx_cmaes_recombine")
        xmean = self.xmean = self.d_xmean.cpu().numpy()
        # ---- evolution paths (cmaes/_cmaes.py:280-287), host vectors ----
        step = xmean - xold
        if self.eigh == "device":  # C^(-1/2) v = B ((B^T v) / D): no n^3 product on the host
            isc_step = np.dot(B, np.dot(B.T, step) / D)
        else:
            isc_step = np.dot(self.invsqrtC, step)
        ps = self.ps = (1.0 - cs) * self.ps + np.sqrt(cs * (2.0 - cs) * mueff) * isc_step / sigma
        cond = np.linalg.norm(ps) / np.sqrt(1.0 - (1.0 - cs) ** (2.0 * (it * P) / P)) / chind < 1.4 + 2.0 / (n + 1.0)
        pc = self.pc
        pc *= 1.0 - cc
        if cond:
            pc += np.sqrt(cc * (2.0 - cc) * mueff) * step / sigma
        # ---- covariance update on the device (cmaes/_cmaes.py:290-295) ----
        self.d_pc.copy_(t.from_numpy(pc), non_blocking=False)
        tmp_coef = 0.0 if cond else c1 * cc * (2.0 - cc)
        _lib.check(L.sx_cmaes_rank_mu(ptr(self.d_arx), ptr(self.d_idx), ptr(self.d_w), mu, ptr(self.d_xold), sigma,
                                      ptr(self.d_pc), c1, cmu, tmp_coef, ptr(self.d_C), ptr(self.d_Y), n, sp), "sx_cmaes_rank_mu")
        # ---- step size (cmaes/_cmaes.py:298) ----
        self.sigma = sigma * np.exp((cs / damps) * (np.linalg.norm(ps) / chind - 1.0))
        # ---- eigendecomposition (cmaes/_cmaes.py:301-309) ----
        due = decomposition_due(it, self.eigeneval, P, c1, cmu, n)
        if not due:
            self.diagC = self.d_C.diagonal().cpu().numpy()
            return B, D
        self.eigeneval = it * P
        _lib.check(L.sx_symmetrize_upper(ptr(self.d_C), n, sp), "sx_symmetrize_upper")
        if self.eigh == "device":
            if self.eig is None:
                self.eig = Eigh(ctx, n)
            # ascending eigenvalues, eigenvectors in columns; from the second time on, started from the last ones
            Dt, _ = self.eig(self.d_C, B=self.d_B, max_sweeps=self.eig_sweeps, start=self.d_B if due == 2 else None,
                             tol=max(1.0e-14, n * 1.1102230246251565e-16),  # LAPACK's own backward error, n * eps
                             refine=os.environ.get("SX_EIGH_REFINE", "1") != "0")  # as the device-resident loop does
            t.sqrt(Dt, out=self.d_D)
            D = self.D = self.d_D.cpu().numpy()
            used, ok, _off = self.eig.info()
            if due == 1:  # what the cold start needed says nothing about the warm ones
                self.eig_sweeps = WARM_SWEEPS0
            else:
                self.eig_sweeps = min(60, used + 1) if ok else 60
            B = self.B = self.d_B.cpu().numpy()
            self.diagC = self.d_C.diagonal().cpu().numpy()
        else:  # host LAPACK, as in the reference, or the caller's solver
            Ch = self.d_C.cpu().numpy()
            D, B = self.eigh(Ch) if callable(self.eigh) else np.linalg.eigh(Ch)
            D, B = np.asarray(D, dtype=np.float64), np.asarray(B, dtype=np.float64)
            o = np.argsort(D)
            D = D[o]
            B = self.B = B[:, o]
            D = self.D = np.sqrt(D)
            self.invsqrtC = np.dot(np.dot(B, np.diag(1.0 / D)), B.T)
            self._put(self.d_B, B)
            self._put(self.d_D, D)
            self.diagC = np.diag(Ch).copy()
        return B, D


register("cmaes", minimize)
