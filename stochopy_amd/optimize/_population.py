"""The run driver DE (_de.py) and PSO / CPSO (_cpso.py) share: sharding prologue, exchange negotiation, graph capture,
the chained kernels' graph cache and state reads, the views handed to callbacks and return_all, the generation loop and
the result.  What differs between the methods is left to hooks of the subclasses: `_setup`, `_population`, `_generation`,
`_after_generation`, `_enqueue_external`, `_enqueue_and_look`, `_best_row`, `_settle_status`; a run that sets `chain` (DE)
also gives `_chain_launch`, `_create_chain_graph` and `_chain_plan`."""
import os

import numpy as np

from .. import _device, _lib
from . import _common
from ._helpers import OptimizeResult

_CAPTURE_MODE = "thread_local"  # see parallel.World.CAPTURE_MODE: torch's NCCL watchdog may poll events while we capture
_CAPTURE_FAILED = {"_rccl_graph_note": "graph capture of the rccl path failed",
                   "_ext_graph_note": "graph capture around the objective failed"}


class _PopulationRun:
    MEMBERS, WHOLE = "individuals", "population"  # (words of the messages)
    CHECK_EVERY = 32  # generations between two looks at the device state when return_all keeps its history on the device
    chain = False     # one kernel per generation (DE sets it per run; PSO has no such kernel)

    def __init__(self, method, fun_id, lower, upper, x0, maxiter, P, xtol, ftol, return_all, verbosity, callback, rng, seed,
                 workers, immediate):
        self.fun_id, self.lower, self.upper = fun_id, lower, upper
        # a caller-supplied objective (factory.batched) cannot be fused: propose / move -> fun -> select
        self.external = None if isinstance(fun_id, int) else fun_id
        self.maxiter, self.P, self.n = maxiter, P, len(lower)
        self.xtol, self.ftol = xtol, ftol
        self.return_all, self.verbosity, self.callback = return_all, verbosity, callback
        self.rng, self.seed = rng, seed
        self.x0 = x0
        self.world = None
        self.Ptotal = P
        self.row0 = 0
        self.immediate = immediate  # one sequential sweep per generation (csrc/sx_async.hip, csrc/sx_async_pso.hip)
        # (what close() releases)
        self.px = None
        self._graph = None
        self._chain_graphs = {}
        self._rccl_graph, self._rccl_graphs, self._rccl_graph_note = None, {}, None
        self._ext_graphs, self._ext_graph_note = {}, None
        self.launches = 0
        if workers != 1 and rng != "philox":
            workers = _common.replicated_workers(method, workers, f'rng="numpy-legacy" replays ONE host stream in the order of '
                                                 f'the whole {self.WHOLE} (rng="philox" shards: draws keyed by the global row)')
        if workers != 1 or os.environ.get("SX_FORCE_SHARDED") == "1":  # the env switch lets a 1-rank group
            from ..parallel import require_world                         # exercise the exchange path (tests)

            self.world = require_world(workers)
            if rng != "philox":
                raise ValueError('a sharded run needs rng="philox" (draws keyed by the global row; see parallel.py)')
            self.row0, self.P = self.world.shard(P)  # this rank's rows; self.P is the LOCAL population from here on
            if immediate:
                raise ValueError("immediate updating is a single-GPU sweep")
        if immediate and self.external is not None:
            raise ValueError(f"immediate updating evaluates {self.MEMBERS} one by one inside the sweep kernel: "
                             "only the factory objectives can do that")

    def _negotiate_exchange(self, requested=None):
        """How the per-generation global best of a sharded run travels: peer writes over xGMI (parallel.PeerExchange) when
        `requested` (None: $SX_EXCHANGE, default "auto") is not "rccl" and that transport passes its self-test on every
        rank, else one all-gather per generation.  Returns (px, exchange, exchange_note); "p2p" that fails raises."""
        if self.world is None:
            return None, None, None
        what = 'exchange="p2p"'
        if requested is None:
            requested, what = os.environ.get("SX_EXCHANGE", "auto"), "SX_EXCHANGE=p2p"
        if requested == "rccl":
            return None, "rccl", None
        from ..parallel import PeerExchange

        px, note = PeerExchange.negotiate(self.ctx, self.world, self.n, float(os.environ.get("SX_XCHG_TIMEOUT_S", "20")))
        if px is None and requested == "p2p":
            raise RuntimeError(f"{what} is not available: {note}")
        return px, ("rccl" if px is None else "p2p"), note

    def _autorun(self):
        t = _device.torch()
        with t.cuda.stream(self.ctx.stream):
            ok = False
            try:
                self._run()
                ok = True
            finally:
                try:
                    if self.px is not None:
                        # Peers may still be reading this rank's exchange / population memory (their last kernels,
                        # remote donor rows): nobody unmaps or frees anything before EVERY rank has drained its
                        # stream.  The meeting point is reached by failing ranks too (it carries a success flag):
                        # a rank whose objective / callback raised makes its peers raise, not hang in a barrier.
                        if ok:
                            self.ctx.sync()
                        if not self.world.all_agree(ok) and ok:
                            raise RuntimeError("a peer rank failed during the run (its own exception says why)")
                finally:
                    self.close()

    def close(self):
        graphs = [g for g in [self._graph, *self._chain_graphs.values()] if g is not None]
        if graphs or self._rccl_graph is not None or self._rccl_graphs or self._ext_graphs or self.px is not None:
            self.ctx.sync()
        self._rccl_graph, self._rccl_graphs, self._ext_graphs = None, {}, {}
        for g in graphs:
            self.ctx.L.sx_graph_destroy(g)
        self._graph, self._chain_graphs = None, {}
        if self.px is not None:
            self.px.close()
            self.px = None

    def _capture(self, n, body, note_attr):
        """`n` calls of `body` captured into one graph, or None when that fails (capture is an optimisation, never a
        requirement): the reason goes to self.<note_attr>, which the caller checks before trying again."""
        t = _device.torch()
        try:
            self.ctx.sync()
            if self.world is not None:
                self.world.quiesce_for_capture(self.ctx)
            g = t.cuda.CUDAGraph()
            with t.cuda.graph(g, stream=self.ctx.stream, capture_error_mode=_CAPTURE_MODE):
                for _ in range(n):
                    body()
            return g
        except Exception as e:
            setattr(self, note_attr, f"{_CAPTURE_FAILED[note_attr]}: {e}")
            return None

    # ---- chained mode (one kernel per generation; the best / termination step of a generation runs in the next launch's
    #      prologue, so the state and the records come in two parities) ----
    def _chain_graph(self, par, size):
        g = self._chain_graphs.get((par, size))
        if g is None:
            g = self._chain_graphs[par, size] = self._create_chain_graph(par, size)
        return g

    def _enqueue_chain(self, ngen):
        ctx = self.ctx
        for size in self._chain_plan(ngen):  # graph lengths, 0 = one eager launch
            par = self.launches & 1
            if size == 0:
                self._chain_launch(par, 0)
                self.launches += 1
            else:
                _lib.check(ctx.L.sx_graph_launch(self._chain_graph(par, size), ctx.stream_ptr), "sx_graph_launch")
                self.launches += size

    def read_state(self):
        """Host view of the run: (chained mode) finalise the last generation into state[2], then read it."""
        if self.chain:
            self._chain_launch(self.launches & 1, 1)
            st = self.ctx.read_state(self.state[16:24])
        else:
            st = self.ctx.read_state(self.state)
        if self.px is not None and self.px.failed():
            raise RuntimeError("peer exchange timed out: a rank did not reach the generation the others "
                               "were waiting for (SX_XCHG_TIMEOUT_S)")
        return st

    # --------------------------------------------------------------- helpers
    def _whole_population(self, it):
        """(population, candidate fitness) of generation `it` as the caller sees them: with workers > 1 every
        rank gathers all shards (callbacks / return_all only -- the reference's parallel backends also hand the
        whole population to the callback on every rank)."""
        X = self._population(it)
        if self.world is None:
            return X, self.candfit
        self.world.all_gather_rows(X, self.Xfull)
        self.world.all_gather_rows(self.candfit, self.candfull)
        return self.Xfull, self.candfull

    def _record(self, it):
        """return_all bookkeeping for generation `it` (de/_de.py:270-278, cpso/_cpso.py:283-295)."""
        if not self.return_all:
            return
        X, cand = self._whole_population(it)
        if self.nout > 0:
            self.xall[it - 1].copy_(X[: self.nout])
            self.funall[it - 1].copy_(cand[: self.nout])  # candidate fitness, de/_de.py:270-273
        else:
            k = int(cand.argmin())
            self.xall[it - 1, 0].copy_(X[k])
            self.funall[it - 1, 0] = cand[k]

    def _partial_result(self, st):
        res = OptimizeResult(x=self._best_row(st), fun=st.gfit, nfev=st.it * self.Ptotal, nit=st.it)
        if self.return_all:
            res.update({"xall": self.xall[: st.it].cpu().numpy(), "funall": self.funall[: st.it].cpu().numpy()})
        return res

    def _after_generation(self, it):
        """Host-visible work between generation `it` and the next (CPSO: the competitive restart)."""

    # ------------------------------------------------------------------ loop
    def _run(self):
        self._setup()
        st = self.st
        if self.callback is not None:
            self.callback(self._whole_population(1)[0].cpu().numpy(), self._partial_result(st))
        # return_all with in-kernel draws: the per-generation history copies (de/_de.py:270-278) are device-side
        # and ordered on the engine stream, so the host need not look at every generation
        record_async = (self.return_all and self.rng == "philox" and self.callback is None and self.nout > 0
                        and self.maxiter > 1)
        stepwise = (self.rng == "numpy-legacy" or self.callback is not None or self.return_all) and not record_async
        while not st.done:
            # maxiter <= 1: the reference still runs one generation before it tests `it >= maxiter`
            remaining = max(self.maxiter - st.it, 1)
            if record_async:
                for j in range(min(remaining, self.CHECK_EVERY)):
                    self._generation()
                    self._record(st.it + 1 + j)  # generations after convergence are no-ops; their slots are cut off
                    self._after_generation(st.it + 1 + j)
                st = self.read_state()
            elif stepwise:
                self._generation()
                self._record(st.it + 1)
                st = self.read_state()
                if self.callback is not None:
                    self.callback(self._whole_population(st.it)[0].cpu().numpy(), self._partial_result(st))
                if not st.done:
                    self._after_generation(st.it)
            elif self.immediate:  # sweeps are long (P sequential individuals): look after every few of them
                for j in range(min(remaining, 8)):
                    self._generation()
                    self._after_generation(st.it + 1 + j)
                st = self.read_state()
            elif self.external is not None:  # kernels and the caller's objective, queued on the engine stream
                self._enqueue_external(remaining)
                st = self.read_state()
            else:
                st = self._enqueue_and_look(st, remaining)
        self.st = st
        status = self._settle_status(st)
        res = OptimizeResult(
            x=self._best_row(st),
            success=status >= 0,
            status=status,
            message=_common.messages[status],
            fun=float(st.gfit),
            nfev=int(st.it) * self.Ptotal,
            nit=int(st.it),
        )
        if self.return_all:
            res.update({"xall": self.xall[: st.it].cpu().numpy(), "funall": self.funall[: st.it].cpu().numpy()})
        # the reference works in place on x0 where its population update does (see x0_in_place)
        if self.x0_in_place and isinstance(self.x0, np.ndarray) and self.x0.dtype == np.float64:
            self.x0[...] = self._population(st.it).cpu().numpy()
        if self.rng == "numpy-legacy":
            self.stream.sync_back()
        self.ctx.sync()
        # (peer exchange: the one meeting point of all ranks -- success flag included -- is `all_agree` in _autorun's
        #  `finally`; a barrier here would pair with a failing rank's all_gather there: mismatched collectives)
        self._res = res

    def result(self):
        return self._res
