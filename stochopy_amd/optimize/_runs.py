"""``options["runs"] = R``: the host path the batched methods share (de, pso / cpso, cmaes, vdcma) -- the option's
validation, the refusals, the seed rule, the batch that one ``sx_*_runs_launch`` takes, and the result.  A method module
keeps the one function that builds its batch (its constants, its inputs, its struct fields) and its own refusals.
``RowwiseBatch`` is the device-memory batch DE and PSO share around a caller's row-wise objective.
"""
import ctypes as C
import warnings

import numpy as np

from .. import _device, _lib, _rng
from . import _common
from ._helpers import OptimizeResult


def batched(runs):
    """Validate ``runs``; is this call a batch (R >= 2)?"""
    if runs is not None and (not isinstance(runs, (int, np.integer)) or isinstance(runs, bool) or runs < 1):
        raise ValueError(f"runs={runs!r}: expected the number of independent runs, an integer >= 1")
    return runs is not None and runs > 1


def per_run(name, value, runs, lo=None, hi=None, positive=False):
    """A hyperparameter that one run of a batch may have to itself.  A scalar (a 0-d array, a numpy scalar) gets the
    reference's check -- a bare ValueError, where the caller stands in the order of checks -- and comes back as it is.  A
    sequence is a sweep: ``runs`` values, run r uses element r; it comes back as an ``(R,)`` float64 array, or the
    ValueError names ``runs``, the option and, where one element is at fault, its index."""
    if _is_scalar(value):
        if (value <= 0.0) if positive else (not lo <= value <= hi):
            raise ValueError()
        return value
    values = _sweep_elements(name, value, runs)
    allowed = "> 0" if positive else f"in [{lo:g}, {hi:g}]"
    out = np.empty(len(values))
    for r, v in enumerate(values):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"runs={runs}: {name}[{r}] = {v!r} is not a number")
        if not np.isfinite(v):
            raise ValueError(f"runs={runs}: {name}[{r}] = {v!r} is not finite")
        if (v <= 0.0) if positive else (not lo <= v <= hi):
            raise ValueError(f"runs={runs}: {name}[{r}] = {v!r}: expected a value {allowed}")
        out[r] = v
    return out


def per_run_names(name, value, runs, table):
    """``per_run`` for an option that is a name out of ``table`` (DE's ``strategy``): a KeyError for an unknown name, as for
    the scalar; a sequence comes back as an ``(R,)`` array of names."""
    if _is_scalar(value):
        if value not in table:
            raise KeyError(value)
        return value
    values = _sweep_elements(name, value, runs)
    for v in values:
        if not isinstance(v, str) or v not in table:
            raise KeyError(v)
    return np.array([str(v) for v in values])


def _is_scalar(value):
    """Not a sequence: what the reference's own comparison is left to deal with (a ragged list has no shape: a sequence)."""
    try:
        return np.ndim(value) == 0
    except ValueError:
        return False


def _sweep_elements(name, value, runs):
    """The R elements of a per-run option as Python / numpy scalars, or a ValueError that names ``runs`` and the option."""
    if not batched(runs):
        raise ValueError(f"{name} is a sequence, one value per run: that needs runs >= 2 (runs={runs!r}); a single run takes "
                         "a scalar")
    try:
        shape = np.shape(value)
    except ValueError:
        shape = None
    if shape is None or len(shape) != 1:
        raise ValueError(f"runs={runs}: {name} must be a scalar or a 1-D sequence of {runs} values, one per run"
                         + ("" if shape is None else f" (its shape is {shape})"))
    if shape[0] != runs:
        raise ValueError(f"runs={runs}: {name} has {shape[0]} values, expected one per run")
    return list(value)


def is_swept(value):
    """Did ``per_run`` / ``per_run_names`` hand back a sweep?"""
    return isinstance(value, np.ndarray) and value.ndim == 1


def setting(value):
    """What a method's ``_minimize_runs`` takes for a hyperparameter: a float, or the sweep's ``(R,)`` array."""
    return value if is_swept(value) else float(value)


def rowwise(fun_id):
    """Is the objective a caller's own that declared ``factory.batched(f, rowwise=True)``?"""
    return not isinstance(fun_id, int) and getattr(fun_id, "rowwise", False) is True


def refuse_common(rng, fun_id, workers, callback, return_all, serves_rowwise=False):
    """What no batched method serves: a run lives in one kernel on one GPU.  ``serves_rowwise``: the calling method has a
    device-memory path around a caller's row-wise objective (de, pso: ``RowwiseBatch``); the others refuse those too."""
    if rng != "philox":
        raise ValueError('runs > 1 needs rng="philox": a run is told apart by its Philox key (in-kernel, counter-based draws)')
    if not isinstance(fun_id, int):
        if not rowwise(fun_id):
            raise ValueError("runs > 1 needs a stochopy_amd.factory objective: it is evaluated inside the run's kernel "
                             "(factory.batched and plain callables run between kernels) -- or, for de and pso, an objective "
                             "declared factory.batched(f, rowwise=True): the rows of all runs are handed over in one call, "
                             "which is only correct when the value of a row depends on that row alone")
        if not serves_rowwise:
            raise ValueError("runs > 1 around a factory.batched(f, rowwise=True) objective is served by de and pso (cpso: "
                             "without the competitive restart); this method needs a stochopy_amd.factory objective, which "
                             "is evaluated inside the run's kernel")
    if workers not in (None, 1):
        raise ValueError(f"runs > 1 uses one GPU (workers={workers})")
    if callback is not None:
        raise ValueError("runs > 1 takes no callback: a run never leaves its kernel")
    if return_all:
        raise ValueError("runs > 1 keeps no history (return_all=True): a run never leaves its kernel")


def refuse_immediate(updating, strict_updating, citation):
    """DE, PSO: ``updating="immediate"`` is refused (strict) or deferred with a warning that points at the line that called
    the method's ``minimize`` (this function <- ``_minimize_runs`` <- ``minimize`` <- that line)."""
    if updating == "immediate":
        if strict_updating:
            raise ValueError('strict_updating=True: updating="immediate" is an ordered sweep; runs > 1 are whole generations in '
                             'parallel (updating="deferred")')
        if strict_updating is None:
            warnings.warn('stochopy_amd: updating="immediate" is an ordered sweep of ONE run; runs > 1 use "deferred" updating, '
                          f"as a parallel backend of the reference does ({citation}).", RuntimeWarning, stacklevel=4)


def refuse_constraints(constraints):
    """CMA-ES, VD-CMA."""
    if constraints is not None:
        raise ValueError(f"runs > 1 serves constraints=None (constraints={constraints!r}: the boundary-weight bookkeeping "
                         "is not part of the run's kernel)")


def refuse_maxiter(maxiter):
    """CMA-ES, VD-CMA: generation 1 is inside the loop."""
    if maxiter < 1:
        raise ValueError(f"runs > 1 needs maxiter >= 1 (maxiter={maxiter})")


def seeds_of(R, seed):
    """An integer s gives s + r to run r; a sequence of R integers is taken as given."""
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        return [int(seed) + r for r in range(R)]
    if seed is not None and np.ndim(seed) == 1 and len(seed) == R:
        return [int(s) for s in seed]
    raise ValueError(f"runs={R} needs seed = an integer s (run r uses s + r) or a sequence of {R} integers")


def standardised(lower, upper, x0, R):
    """CMA-ES, VD-CMA: xm, xstd of the box and the caller's ``x0`` -- (n,) for all runs or (R, n) -- in the model's
    coordinates, (R, n); None without an ``x0``."""
    xm, xstd = 0.5 * (upper + lower), 0.5 * (upper - lower)
    if x0 is None:
        return xm, xstd, None
    return xm, xstd, np.ascontiguousarray(np.broadcast_to((np.asarray(x0, dtype=np.float64) - xm) / xstd, (R, len(lower))))


def set_model_scalars(a, n, mu, fun_id, maxiter, sigma, xtol, ftol):
    """CMA-ES, VD-CMA: the struct fields the two share (``ilim``: cmaes/_cmaes.py:221)."""
    a.n, a.mu, a.fun_id, a.maxiter = n, mu, fun_id, maxiter
    a.ilim = int(10.0 + 30.0 * n / a.P)
    a.sigma = a.insigma = sigma
    a.xtol, a.ftol = xtol, ftol


class Batch:
    """R runs for one ``sx_*_runs_launch``: the device context, the argument struct ``a`` and ``dev``, the device tensors its
    pointers name (inputs, outputs, workspace).  Pointers that are never bound stay NULL."""

    # the per-run arrays of sx_*_runs_sweep_launch, in the order of its arguments
    SWEEP = {"sx_de_runs_launch": ("F", "CR", "strategy"), "sx_pso_runs_launch": ("w", "c1", "c2", "gamma"),
             "sx_cma_runs_launch": ("sigma",), "sx_vd_runs_launch": ("sigma",)}

    def __init__(self, entry, args, seeds, P):
        self.entry, self.a, self.seeds, self.R, self.P = entry, args, seeds, len(seeds), P
        self.ctx = _device.Context()
        self.dev, self.out, self.sweep = {}, (), {}
        args.R, args.P = self.R, P

    def stream(self):
        """Uploads, fills and read-backs go inside ``with batch.stream():``."""
        return _device.torch().cuda.stream(self.ctx.stream)

    def bind(self, **tensors):
        for name, tensor in tensors.items():
            self.dev[name] = tensor
            setattr(self.a, name, tensor.data_ptr())

    def bind_sweep(self, **settings):
        """Of ``settings`` (argument name of the ``_sweep_`` entry -> float, or (R,) array), upload the arrays: run r reads
        element r of those, and the struct's scalar for the rest.  Returns the scalars, for the struct -- of a swept
        setting, run 0's: the launch checks the struct's fields whether or not an array replaces them."""
        scalars = {}
        for name, value in settings.items():
            if is_swept(value):
                if name not in self.SWEEP[self.entry] or value.shape != (self.R,):
                    raise ValueError(f"{self.entry}: no per-run {name} of shape {value.shape} for {self.R} runs")
                dtype = np.int32 if name == "strategy" else np.float64
                self.sweep[name] = self.ctx.upload_async(np.ascontiguousarray(value, dtype=dtype))
                scalars[name] = value[0].item()
            else:
                scalars[name] = value
        return scalars

    def upload_keys(self):
        keys = np.array([_rng.philox_key(s) for s in self.seeds], dtype=np.uint32)
        self.bind(keys=self.ctx.upload_async(keys.view(np.int32)))

    def outputs(self, n, optional, wanted, extra=()):
        """xs, funs, nits, statuses, the method's ``extra`` per-run doubles, and those of ``optional`` (name -> (shape,
        dtype); None: double) that ``wanted`` names."""
        t, R = _device.torch(), self.R
        spec = {"xs": ((R, n), None), "funs": ((R,), None), "nits": ((R,), t.int64), "statuses": ((R,), t.int32)}
        spec.update({name: ((R,), None) for name in extra})
        spec.update({name: optional[name] for name in wanted})
        for name in ("xs", "funs", *extra, "nits", "statuses", *wanted):
            self.bind(**{name: self.ctx.empty(*spec[name])})
        self.out = ("xs", "funs", "nits", "statuses", *extra, *wanted)

    def launch(self):
        if not self.sweep:
            _lib.check(getattr(self.ctx.L, self.entry)(C.byref(self.a), self.ctx.stream_ptr), self.entry)
            return
        entry = self.entry.replace("_launch", "_sweep_launch")
        arrays = [self.sweep[name].data_ptr() if name in self.sweep else None for name in self.SWEEP[self.entry]]
        _lib.check(getattr(self.ctx.L, entry)(C.byref(self.a), *arrays, self.ctx.stream_ptr), entry)

    def fetch(self):
        """The outputs as numpy arrays, by name."""
        with self.stream():
            return {name: self.dev[name].cpu().numpy() for name in self.out}


class RowwiseBatch(Batch):
    """R runs of DE or PSO around a caller's row-wise objective (``factory.batched(f, rowwise=True)``), in device memory
    (csrc/sx_runs_unfused.hip): three ``(R, P, n)`` populations, the per-run states and best rows, the records of the
    selection.  There is no LDS limit.  A generation of ALL runs is the method's propose / move kernel, ONE call of the
    objective on the stacked ``(R * P, n)`` rows, the selection kernel and one best / termination workgroup per run.  A run
    that has ended is frozen -- its workgroups return at entry -- and the objective still receives its last candidate rows
    until every run has ended.  ``entry`` is the method's propose / move entry point; a method module sets its own struct
    fields and sweep arrays, then ``launch()`` and ``fetch()`` as with a ``Batch``."""

    # the per-run arrays of the propose / move entries, in the order of their arguments
    SWEEP = {"sx_runs_rowwise_de_propose": ("F", "CR", "strategy"), "sx_runs_rowwise_pso_move": ("w", "c1", "c2")}
    # entry -> (sx_runs_rowwise_args.method, the population the objective is handed: DE's candidates, PSO's positions)
    KINDS = {"sx_runs_rowwise_de_propose": (0, "pop2"), "sx_runs_rowwise_pso_move": (1, "pop0")}

    def __init__(self, entry, external, seeds, lower, upper, x0, maxiter, P, constrained, xtol, ftol):
        super().__init__(entry, _lib.SxRunsRowwiseArgs(), seeds, P)
        a, ctx, R, t = self.a, self.ctx, self.R, _device.torch()
        n = self.n = len(lower)
        self.external, self.maxiter = external, maxiter
        per_run = int(ctx.L.sx_runs_rowwise_partials(P, n))
        with self.stream():
            self.upload_keys()
            d_bounds = ctx.upload_async(np.concatenate([lower, upper]))
            self.bind(lower=d_bounds[:n], upper=d_bounds[n:])
            if x0 is not None:
                self.bind(x0=ctx.upload(np.array(x0, dtype=np.float64)))
                a.x0_stride = P * n if self.dev["x0"].dim() == 3 else 0
            self.bind(pop0=ctx.empty((R, P, n)), pop1=ctx.empty((R, P, n)), pop2=ctx.empty((R, P, n)),
                      fit=ctx.empty((R * P,)), candfit=ctx.empty((R * P,)), state=ctx.zeros((R, 8), dtype=t.int64),
                      gbest=ctx.empty((R, n)), part_f=ctx.empty((R, per_run)), part_i=ctx.empty((R, per_run), dtype=t.int64),
                      ended=ctx.zeros((1,), dtype=t.int32))
            self.outputs(n, {}, ())
        a.n, a.method, a.constraints, a.maxiter, a.xtol, a.ftol = n, self.KINDS[entry][0], int(constrained), maxiter, xtol, ftol

    def _evaluate(self, X):
        """One call of the objective on all runs' rows; the kernels read its values where it left them (no copy)."""
        f = self.dev["f"] = self.external(self.ctx, X)  # (kept until the next call: the kernels that read it are enqueued by then)
        self.a.f = f.data_ptr()

    def launch(self):
        """All runs, from the initial populations to each run's own termination.  Generations are enqueued eagerly on the
        engine stream, ``_PopulationRun.CHECK_EVERY`` at a time (fewer when ``maxiter`` leaves fewer); then one 4-byte
        read-back tells whether any run is still active."""
        from ._population import _PopulationRun

        L, a, sp, R, move = self.ctx.L, C.byref(self.a), self.ctx.stream_ptr, self.R, self.entry
        X = self.dev[self.KINDS[move][1]].view(R * self.P, self.n)
        sweep = [self.sweep[name].data_ptr() if name in self.sweep else None for name in self.SWEEP[move]]
        strategy = self.sweep["strategy"].data_ptr() if "strategy" in self.sweep else None
        with self.stream():
            _lib.check(L.sx_runs_rowwise_init(a, sp), "sx_runs_rowwise_init")
            self._evaluate(X)
            _lib.check(L.sx_runs_rowwise_start(a, strategy, sp), "sx_runs_rowwise_start")
            it = 1  # the generation every run that is still active holds
            while True:
                # maxiter <= 1: the reference still runs one generation before it tests `it >= maxiter`
                for _ in range(min(max(self.maxiter - it, 1), _PopulationRun.CHECK_EVERY)):
                    _lib.check(getattr(L, move)(a, *sweep, sp), move)
                    self._evaluate(X)
                    _lib.check(L.sx_runs_rowwise_select(a, sp), "sx_runs_rowwise_select")
                    _lib.check(L.sx_runs_rowwise_finalize(a, sp), "sx_runs_rowwise_finalize")
                    it += 1
                if int(self.dev["ended"].cpu()[0]) >= R:  # (generations enqueued for a run that has ended are no-ops)
                    break


def result(out, P, **settings):
    """The best run (``np.argmin``) as the result, with every run's outputs beside it; ``sweep``: of ``settings`` (option
    name -> what ``_minimize_runs`` got), those that were per run, if any."""
    sweep = {name: np.array(value) for name, value in settings.items() if is_swept(value)}
    if sweep:
        out = dict(out, sweep=sweep)
    xs, funs, nits, statuses = out["xs"], out["funs"], out["nits"], out["statuses"]
    best = int(np.argmin(funs))
    status = int(statuses[best])
    return OptimizeResult(x=xs[best].copy(), success=status >= 0, status=status, message=_common.messages[status],
                          fun=float(funs[best]), nfev=int(nits.sum()) * P, nit=int(nits[best]), run=best, **out)
