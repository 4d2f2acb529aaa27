#!/usr/bin/env python3
"""Throughput of many independent PSO / CPSO runs in one launch (options["runs"], csrc/sx_pso_runs.hip) on one MI355X, next to
the only way to do the same work without it: a Python loop of single minimize() calls.

Workload: ackley, n = 32, popsize = 32, maxiter = 200, tolerances that never trigger (every run does its 200 generations),
Philox draws, deferred updating; PSO, and CPSO with competitivity 1.
    runs R in {256, 4096, 16384}   ONE sx_pso_runs_launch of R workgroups; time = device events around a round's launches
                                   (each a whole batch from the initial swarm, repeated back to back for ~--window seconds),
                                   divided by their number.  "call" is the wall time of one whole minimize(..., runs=R) call on
                                   top: uploads, launch, results back on the host.
    loop                           --loop-calls (64) single minimize() calls with the same settings and seeds s, s+1, ..., wall
                                   time with the stream drained at the end.  The loop's rate does not depend on how many runs
                                   are asked for: the figure beside R runs IS this rate, not a measurement of R calls.
Everything is warmed up once, then the configurations take turns for --rounds rounds; a line gives the median and the spread
(min .. max) of its rounds, in objective evaluations per second (nit x popsize per run).

    python tools/bench_pso_runs.py [--rounds 5] [--window 0.25] [--loop-calls 64] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, P, MAXITER, SEED = 32, 32, 200, 3
RUNS = (256, 4096, 16384)
METHODS = {"pso": 0.0, "cpso": 1.0}  # competitivity
W, C1, C2 = 0.7298, 1.49618, 1.49618
OPTS = {"popsize": P, "maxiter": MAXITER, "xtol": 0.0, "ftol": -1.0, "rng": "philox", "updating": "deferred", "backend": "hip"}
BOUNDS = [[-5.12, 5.12]] * N


class DeviceBatch:
    """The buffers and arguments of one batch, launched as optimize.minimize(..., runs=R) does."""

    def __init__(self, ctx, method, R):
        from stochopy_amd import _device, _lib, _rng

        t = _device.torch()
        self.ctx, self.L, self.R, self.method = ctx, ctx.L, R, method
        keys = np.array([_rng.philox_key(SEED + r) for r in range(R)], dtype=np.uint32)
        self.dev = dev = {"keys": ctx.upload(keys.view(np.int32)), "lower": ctx.upload(np.full(N, -5.12)),
                          "upper": ctx.upload(np.full(N, 5.12)), "xs": ctx.empty((R, N)), "funs": ctx.empty((R,)),
                          "nits": ctx.empty((R,), dtype=t.int64), "statuses": ctx.empty((R,), dtype=t.int32)}
        self.a = a = _lib.SxPsoRunsArgs()
        for name in dev:
            setattr(a, name, _device.ptr(dev[name]))
        a.R, a.P, a.x0_stride, a.n = R, P, 0, N
        a.fun_id, a.constraints, a.maxiter = _lib.FUN_IDS["ackley"], 0, MAXITER
        a.w, a.c1, a.c2, a.gamma = W, C1, C2, METHODS[method]
        a.delta = float(np.log(1.0 + 0.003 * P) / np.max((0.2, np.log(0.01 * MAXITER)))) if a.gamma else 0.0
        a.xtol, a.ftol = OPTS["xtol"], OPTS["ftol"]
        self.evals = R * MAXITER * P

    def timed(self, launches=1):
        """Seconds per launch (a whole batch), over `launches` launches back to back."""
        from stochopy_amd import _lib

        t = __import__("torch")
        with t.cuda.stream(self.ctx.stream):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                _lib.check(self.L.sx_pso_runs_launch(C.byref(self.a), self.ctx.stream_ptr), "sx_pso_runs_launch")
            e1.record()
            e1.synchronize()
        assert int(self.dev["nits"].min()) == MAXITER  # every run did all its generations
        return e0.elapsed_time(e1) * 1e-3 / launches


def options(method, **more):
    return dict(OPTS, **({"competitivity": METHODS[method]} if method == "cpso" else {}), **more)


def whole_call(sa, method, R):
    """Wall seconds of one minimize(..., runs=R) call."""
    t0 = time.perf_counter()
    res = sa.optimize.minimize(sa.factory.ackley, BOUNDS, method=method, options=options(method, seed=SEED, runs=R))
    dt = time.perf_counter() - t0
    assert res.nfev == R * MAXITER * P
    return dt


def loop_of_calls(sa, ctx, method, calls):
    """Wall seconds per call of `calls` single minimize() calls, one after the other."""
    t0 = time.perf_counter()
    for r in range(calls):
        res = sa.optimize.minimize(sa.factory.ackley, BOUNDS, method=method, options=options(method, seed=SEED + r))
        assert res.nit == MAXITER
    ctx.sync()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per timed round")
    ap.add_argument("--loop-calls", type=int, default=64)
    ap.add_argument("--out")
    args = ap.parse_args()
    import stochopy_amd as sa
    from stochopy_amd import _device

    ctx = _device.Context()
    batches = [DeviceBatch(ctx, method, R) for method in METHODS for R in RUNS]
    launches = {}
    for b in batches:
        b.timed()  # warm-up: code object load
        launches[b] = max(1, int(round(args.window / b.timed())))
        whole_call(sa, b.method, b.R)
    for method in METHODS:
        loop_of_calls(sa, ctx, method, 8)  # warm-up: graphs of the generation kernels, allocator
    times, calls = {b: [] for b in batches}, {b: [] for b in batches}
    loop = {method: [] for method in METHODS}
    for _ in range(args.rounds):
        for b in batches:
            times[b].append(b.timed(launches[b]))
            calls[b].append(whole_call(sa, b.method, b.R))
        for method in METHODS:
            loop[method].append(loop_of_calls(sa, ctx, method, args.loop_calls))
    per_call = MAXITER * P
    lines, loop_rate = [], {}
    for method in METHODS:
        lp = np.array(loop[method])
        loop_rate[method] = per_call / float(np.median(lp))
        lines.append({"config": "loop of single minimize() calls", "method": method, "calls_timed": args.loop_calls,
                      "rounds": args.rounds, "seconds_per_call_median": float(np.median(lp)),
                      "seconds_per_call_min": float(lp.min()), "seconds_per_call_max": float(lp.max()),
                      "us_per_generation": float(np.median(lp)) / MAXITER * 1e6, "evals_per_s": loop_rate[method],
                      "evals_per_s_spread": [per_call / float(lp.max()), per_call / float(lp.min())]})
    for b in batches:
        ts, cs = np.array(times[b]), np.array(calls[b])
        rate = b.evals / float(np.median(ts))
        lines.append({"config": "runs", "method": b.method, "runs": b.R, "ndim": N, "popsize": P, "maxiter": MAXITER,
                      "rounds": args.rounds, "launches_per_round": launches[b], "seconds_median": float(np.median(ts)),
                      "seconds_min": float(ts.min()), "seconds_max": float(ts.max()), "evals_per_s": rate,
                      "evals_per_s_spread": [b.evals / float(ts.max()), b.evals / float(ts.min())],
                      "call_seconds_median": float(np.median(cs)), "call_evals_per_s": b.evals / float(np.median(cs)),
                      "loop_evals_per_s": loop_rate[b.method],
                      "loop_seconds_for_these_runs_at_that_rate": b.R * per_call / loop_rate[b.method],
                      "ratio_kernel_to_loop": rate / loop_rate[b.method],
                      "ratio_call_to_loop": b.evals / float(np.median(cs)) / loop_rate[b.method]})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
