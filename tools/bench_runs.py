#!/usr/bin/env python3
"""Throughput of many independent runs in one launch (options["runs"]; csrc/sx_de_runs.hip, sx_pso_runs.hip, sx_cma_runs.hip,
sx_vd_runs.hip) on one MI355X, next to the only way to do the same work without it: a Python loop of single minimize() calls.

Workloads (WORKLOADS below): maxiter = 200, xtol = 0 and ftol = -1 (rules 0 and 1 never trigger), Philox draws.
    de            rosenbrock, n = 32, popsize = 32, best1bin, deferred updating
    pso, cpso     ackley, n = 32, popsize = 32, deferred updating; cpso with competitivity 1
    cmaes         rosenbrock, two shapes: n = 10, popsize = 10 (the reference's default population 4 + 3 ln n) and n = 32,
                  popsize = 64; a run that another rule ends early is counted with the generations it did
    vdcma         rosenbrock, two shapes: n = 64, popsize = 16 (the default population) and n = 256, popsize = 20
Every run of de, pso, cpso and vdcma must do its 200 generations (checked).
    runs R in {256, 4096, 16384}   ONE sx_*_runs_launch of R workgroups -- the batch minimize(..., runs=R) builds (each method's
                                   _runs_batch), built once and launched again and again; time = device events around a
                                   round's launches (each a whole batch from the start, back to back for ~--window seconds),
                                   divided by their number.  "call" is the wall time of one whole minimize(..., runs=R) call on
                                   top: the host's draws, uploads, launch, results back on the host.
    loop                           --loop-calls (64) single minimize() calls with the same settings and seeds s, s+1, ...,
                                   wall time with the stream drained at the end.  The loop's rate does not depend on how many
                                   runs are asked for: the figure beside R runs IS this rate, not a measurement of R calls.
    --sweep                        the same batches once more with their per-run arrays bound (sx_*_runs_sweep_launch): every
                                   hyperparameter of SWEEPS below spread evenly, run 0 to run R - 1, over the stated interval
                                   around the workload's scalar.  Their lines ("runs, swept") stand beside the uniform ones and
                                   are not compared with them: other settings end other runs at other generations (the share
                                   that did all of them is recorded, not required).
Everything is warmed up once, then the configurations take turns for --rounds rounds; a line gives the median and the spread
(min .. max) of its rounds, in objective evaluations per second (nit x popsize per run).

    --rowwise                      instead of all that (--method de, pso): runs=R around a caller's own row-wise device
                                   objective, factory.batched(f, rowwise=True) -- csrc/sx_runs_unfused.hip -- as whole-call wall
                                   times next to the loop of single minimize(factory.batched(f)) calls and, where it fits, the
                                   resident factory batch (rowwise_main below; shapes: ROWWISE_SHAPES).

    python tools/bench_runs.py [--method de|pso|cpso|cmaes|vdcma ...] [--sweep | --rowwise] [--rounds 5] [--window 0.25] [--loop-calls 64] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAXITER, SEED = 200, 3
RUNS = (256, 4096, 16384)
COMMON = {"maxiter": MAXITER, "xtol": 0.0, "ftol": -1.0, "rng": "philox", "backend": "hip"}
PSO = (0.7298, 1.49618, 1.49618)  # inertia, cognitivity, sociability
# module of stochopy_amd/optimize whose _runs_batch builds the batch; `own`: its arguments between popsize and xtol;
# shapes: (ndim, popsize); half: the box is [-half, half]^ndim; full: every run must do all its generations
WORKLOADS = {
    "de": dict(module="_de", objective="rosenbrock", shapes=((32, 32),), half=5.12, full=True, warm_loop=8,
               own=(0.5, 0.9, "best1bin", None), opts={"strategy": "best1bin", "updating": "deferred"}),
    "pso": dict(module="_cpso", objective="ackley", shapes=((32, 32),), half=5.12, full=True, warm_loop=8,
                own=PSO + (None, None), opts={"updating": "deferred"}),
    "cpso": dict(module="_cpso", objective="ackley", shapes=((32, 32),), half=5.12, full=True, warm_loop=8,
                 own=PSO + (1.0, None), opts={"updating": "deferred", "competitivity": 1.0}),
    "cmaes": dict(module="_cmaes", objective="rosenbrock", shapes=((10, 10), (32, 64)), half=3.0, full=False, warm_loop=4,
                  own=(0.1, 0.5), opts={"sigma": 0.1}),
    "vdcma": dict(module="_vdcma", objective="rosenbrock", shapes=((64, 16), (256, 20)), half=3.0, full=True, warm_loop=4,
                  own=(0.1, 0.5), opts={"sigma": 0.1}),
}
# --sweep: index into `own` -> (option, lowest, highest): run r of R uses lowest + (highest - lowest) r / (R - 1)
SWEEPS = {
    "de": {0: ("mutation", 0.4, 0.6), 1: ("recombination", 0.8, 1.0)},
    "pso": {0: ("inertia", 0.6, 0.8), 1: ("cognitivity", 1.3, 1.7), 2: ("sociability", 1.3, 1.7)},
    "cpso": {0: ("inertia", 0.6, 0.8), 1: ("cognitivity", 1.3, 1.7), 2: ("sociability", 1.3, 1.7),
             3: ("competitivity", 0.8, 1.2)},
    "cmaes": {0: ("sigma", 0.05, 0.2)},
    "vdcma": {0: ("sigma", 0.05, 0.2)},
}


class Config:
    """One method at one shape: the minimize() calls, and the timed batch of R runs."""

    def __init__(self, sa, method, n, P):
        w = WORKLOADS[method]
        self.sa, self.method, self.n, self.P, self.full = sa, method, n, P, w["full"]
        self.fun, self.bounds = getattr(sa.factory, w["objective"]), [[-w["half"], w["half"]]] * n
        self.options = dict(COMMON, popsize=P, **w["opts"])

    def batch(self, R, swept=False):
        from stochopy_amd import _lib

        w = WORKLOADS[self.method]
        own = list(w["own"])
        if swept:
            for k, (_, lo, hi) in SWEEPS[self.method].items():
                own[k] = np.linspace(lo, hi, R)
        build = importlib.import_module("stochopy_amd.optimize." + w["module"])._runs_batch
        return build([SEED + r for r in range(R)], _lib.FUN_IDS[w["objective"]], np.full(self.n, -w["half"]),
                     np.full(self.n, w["half"]), None, MAXITER, self.P, *own, COMMON["xtol"], COMMON["ftol"])

    def minimize(self, **more):
        return self.sa.optimize.minimize(self.fun, self.bounds, method=self.method, options=dict(self.options, **more))

    def whole_call(self, R):
        """Wall seconds of one minimize(..., runs=R) call."""
        t0 = time.perf_counter()
        res = self.minimize(seed=SEED, runs=R)
        dt = time.perf_counter() - t0
        assert res.nfev == int(res.nits.sum()) * self.P and (not self.full or res.nfev == R * MAXITER * self.P)
        return dt

    def loop_of_calls(self, ctx, calls):
        """Wall seconds and evaluations of `calls` single minimize() calls, one after the other."""
        t0 = time.perf_counter()
        evals = 0
        for r in range(calls):
            res = self.minimize(seed=SEED + r)
            assert not self.full or res.nit == MAXITER
            evals += res.nfev
        ctx.sync()
        return time.perf_counter() - t0, evals


def timed(config, batch, launches=1, swept=False):
    """Seconds per launch (a whole batch), over `launches` launches back to back; the evaluations one launch did and the share
    of its runs that did all their generations."""
    t = __import__("torch")
    with batch.stream():
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            batch.launch()
        e1.record()
        e1.synchronize()
    nits = batch.dev["nits"]
    full = float((nits == MAXITER).double().mean())
    assert swept or not config.full or full == 1.0, "a run ended before its %d generations" % MAXITER
    return e0.elapsed_time(e1) * 1e-3 / launches, int(nits.sum()) * config.P, full


# --rowwise: (ndim, popsize, runs, maxiter): README's own shape, and one large shape the resident path refuses
ROWWISE_SHAPES = ((32, 32, 4096, MAXITER), (128, 1024, 64, 50))


def rowwise_objectives(sa, name):
    """objective name -> (device function, factory objective with the same values or None): the library's own sx_eval wrapped
    as a caller's device function (tests/test_gpu_sample_batched.py device_objective), and a quadratic written in torch."""
    import ctypes as C

    t = __import__("torch")
    from stochopy_amd import _lib

    L, fid = _lib.lib(), _lib.FUN_IDS[name]

    def sx_eval(X):
        P, n = X.shape
        f = t.empty((P,), dtype=t.float64, device=X.device)
        assert L.sx_eval(fid, X.data_ptr(), P, n, n, None, None, f.data_ptr(), None, None,
                         C.c_void_p(t.cuda.current_stream().cuda_stream)) == 0
        return f

    def torch_quadratic(X):
        return (X * X).sum(dim=1)

    return {"sx_eval " + name: (sx_eval, getattr(sa.factory, name)), "torch quadratic": (torch_quadratic, None)}


def rowwise_main(args, sa, ctx):
    """--rowwise: whole-call wall times (ending in a synchronise, after a warm-up, the forms alternated) of
        rowwise    minimize(factory.batched(f, rowwise=True), ..., runs=R): R populations in device memory, f once a generation
        loop       --loop-calls single minimize(factory.batched(f)) calls, seeds s, s + 1, ...; the loop's time for R runs is
                   R times its time per call (a rate, as above: not a measurement of R calls)
        resident   with the sx_eval wrapper, where the shape fits the LDS: minimize(factory.<objective>, ..., runs=R), the
                   fused resident batch -- the difference to `rowwise` is the price of unfusing."""
    lines = []
    for method in args.method:
        if method not in ("de", "pso"):
            raise SystemExit("--rowwise serves --method de and --method pso")
        w = WORKLOADS[method]
        for n, P, R, maxiter in ROWWISE_SHAPES:
            bounds = [[-w["half"], w["half"]]] * n
            base = dict(COMMON, popsize=P, maxiter=maxiter, **w["opts"])
            for label, (fun, fused) in rowwise_objectives(sa, w["objective"]).items():
                forms = {"rowwise": lambda: sa.optimize.minimize(sa.factory.batched(fun, rowwise=True), bounds, method=method,
                                                                 options=dict(base, seed=SEED, runs=R))}
                if fused is not None:
                    try:
                        sa.optimize.minimize(fused, bounds, method=method, options=dict(base, seed=SEED, runs=R))
                        forms["resident"] = lambda: sa.optimize.minimize(fused, bounds, method=method,
                                                                         options=dict(base, seed=SEED, runs=R))
                    except ValueError:  # the shape does not fit the LDS
                        pass

                def loop():
                    for r in range(args.loop_calls):
                        sa.optimize.minimize(sa.factory.batched(fun), bounds, method=method, options=dict(base, seed=SEED + r))

                forms["loop"] = loop
                for form in forms.values():  # warm-up: code objects, graphs, allocator
                    form()
                ctx.sync()
                secs = {name: [] for name in forms}
                for _ in range(args.rounds):
                    for name, form in forms.items():
                        t0 = time.perf_counter()
                        res = form()
                        ctx.sync()
                        secs[name].append(time.perf_counter() - t0)
                        assert name == "loop" or (res.nits == maxiter).all()
                evals = R * maxiter * P
                line = {"config": "rowwise", "method": method, "objective": label, "ndim": n, "popsize": P, "runs": R,
                        "maxiter": maxiter, "rounds": args.rounds, "loop_calls_timed": args.loop_calls}
                for name, s in secs.items():
                    s = np.array(s) * (R / args.loop_calls if name == "loop" else 1.0)
                    line.update({name + "_seconds_median": float(np.median(s)), name + "_seconds_min": float(s.min()),
                                 name + "_seconds_max": float(s.max()), name + "_evals_per_s": evals / float(np.median(s))})
                # ratios of median seconds: how many times as long as the row-wise batch the loop takes (above 1: the batch is
                # faster), and how many times as long as the resident batch the row-wise one takes (the price of unfusing)
                line["loop_seconds_over_rowwise_seconds"] = line["loop_seconds_median"] / line["rowwise_seconds_median"]
                if "resident" in secs:
                    line["rowwise_seconds_over_resident_seconds"] = (line["rowwise_seconds_median"]
                                                                     / line["resident_seconds_median"])
                lines.append(line)
                print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--method", nargs="+", choices=sorted(WORKLOADS), default=["de"])
    ap.add_argument("--sweep", action="store_true", help="also time every batch with its per-run arrays bound")
    ap.add_argument("--rowwise", action="store_true",
                    help="time runs=R around a caller's row-wise device objective instead (de, pso): see rowwise_main")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per timed round")
    ap.add_argument("--loop-calls", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    import stochopy_amd as sa
    from stochopy_amd import _device

    ctx = _device.Context()
    if args.rowwise:
        return rowwise_main(args, sa, ctx)
    configs = [Config(sa, method, n, P) for method in args.method for n, P in WORKLOADS[method]["shapes"]]
    batches = [(c, R, c.batch(R)) for c in configs for R in RUNS]
    swept = [(c, R, c.batch(R, swept=True)) for c in configs for R in RUNS] if args.sweep else []
    launches = {}
    for c, R, b in swept:
        timed(c, b, swept=True)
        launches[b] = max(1, int(round(args.window / timed(c, b, swept=True)[0])))
    for c, R, b in batches:
        timed(c, b)  # warm-up: code object load
        launches[b] = max(1, int(round(args.window / timed(c, b)[0])))
        c.whole_call(R)
    for c in configs:
        c.loop_of_calls(ctx, WORKLOADS[c.method]["warm_loop"])  # warm-up: graphs and code objects of the single run, allocator
    times, calls = {b: [] for _, _, b in batches + swept}, {b: [] for _, _, b in batches}
    loop = {c: [] for c in configs}
    for _ in range(args.rounds):
        for c, R, b in batches:
            times[b].append(timed(c, b, launches[b]))
            calls[b].append(c.whole_call(R))
        for c, R, b in swept:
            times[b].append(timed(c, b, launches[b], swept=True))
        for c in configs:
            loop[c].append(c.loop_of_calls(ctx, args.loop_calls))
    lines, loop_rate = [], {}
    for c in configs:
        secs = np.array([s for s, _ in loop[c]])
        rates = np.array([e / s for s, e in loop[c]])
        gens = np.array([e / c.P for _, e in loop[c]])
        loop_rate[c] = float(np.median(rates))
        lines.append({"config": "loop of single minimize() calls", "method": c.method, "ndim": c.n, "popsize": c.P,
                      "calls_timed": args.loop_calls, "rounds": args.rounds,
                      "seconds_per_call_median": float(np.median(secs)) / args.loop_calls,
                      "seconds_per_call_min": float(secs.min()) / args.loop_calls,
                      "seconds_per_call_max": float(secs.max()) / args.loop_calls,
                      "us_per_generation": float(np.median(secs / gens)) * 1e6, "evals_per_s": loop_rate[c],
                      "evals_per_s_spread": [float(rates.min()), float(rates.max())]})
    for c, R, b in batches:
        ts, cs = np.array([s for s, _, _ in times[b]]), np.array(calls[b])
        _, evals, full = times[b][-1]
        rate, lr = evals / float(np.median(ts)), loop_rate[c]
        lines.append({"config": "runs", "method": c.method, "runs": R, "ndim": c.n, "popsize": c.P, "maxiter": MAXITER,
                      "rounds": args.rounds, "launches_per_round": launches[b], "runs_that_did_all_generations": full,
                      "evals_per_launch": evals, "seconds_median": float(np.median(ts)), "seconds_min": float(ts.min()),
                      "seconds_max": float(ts.max()), "evals_per_s": rate,
                      "evals_per_s_spread": [evals / float(ts.max()), evals / float(ts.min())],
                      "call_seconds_median": float(np.median(cs)), "call_seconds_min": float(cs.min()),
                      "call_seconds_max": float(cs.max()), "call_evals_per_s": evals / float(np.median(cs)),
                      "loop_evals_per_s": lr, "loop_seconds_for_these_runs_at_that_rate": evals / lr,
                      "ratio_kernel_to_loop": rate / lr, "ratio_call_to_loop": evals / float(np.median(cs)) / lr})
    for c, R, b in swept:
        ts = np.array([s for s, _, _ in times[b]])
        _, evals, full = times[b][-1]
        lines.append({"config": "runs, swept", "method": c.method, "runs": R, "ndim": c.n, "popsize": c.P, "maxiter": MAXITER,
                      "sweep": {name: [lo, hi] for name, lo, hi in SWEEPS[c.method].values()},
                      "rounds": args.rounds, "launches_per_round": launches[b], "runs_that_did_all_generations": full,
                      "evals_per_launch": evals, "seconds_median": float(np.median(ts)), "seconds_min": float(ts.min()),
                      "seconds_max": float(ts.max()), "evals_per_s": evals / float(np.median(ts)),
                      "evals_per_s_spread": [evals / float(ts.max()), evals / float(ts.min())]})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
