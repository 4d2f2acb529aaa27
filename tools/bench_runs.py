#!/usr/bin/env python3
"""Throughput of many independent DE runs in one launch (options["runs"], csrc/sx_de_runs.hip) on one MI355X, next to the
only way to do the same work without it: a Python loop of single minimize() calls.

Workload: rosenbrock, n = 32, popsize = 32, best1bin, maxiter = 200, tolerances that never trigger (every run does its 200
generations), Philox draws, deferred updating.
    runs R in {256, 4096, 16384}   ONE sx_de_runs_launch of R workgroups; time = device events around a round's launches
                                   (each a whole batch from the initial population, repeated back to back for ~--window
                                   seconds), divided by their number.  "call" is the wall time of one whole
                                   minimize(..., runs=R) call on top: uploads, launch, results back on the host.
    loop                           --loop-calls (64) single minimize() calls with the same settings and seeds s, s+1, ...,
                                   wall time with the stream drained at the end.  The loop's rate does not depend on how many
                                   runs are asked for: the figure beside R runs IS this rate, not a measurement of R calls.
Everything is warmed up once, then the configurations take turns for --rounds rounds; a line gives the median and the spread
(min .. max) of its rounds, in objective evaluations per second (nit x popsize per run).

    python tools/bench_runs.py [--rounds 5] [--window 0.25] [--loop-calls 64] [--out FILE]
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
OPTS = {"popsize": P, "maxiter": MAXITER, "strategy": "best1bin", "xtol": 0.0, "ftol": -1.0, "rng": "philox",
        "updating": "deferred", "backend": "hip"}
BOUNDS = [[-5.12, 5.12]] * N


class DeviceBatch:
    """The buffers and arguments of one batch, launched as optimize.minimize(..., runs=R) does."""

    def __init__(self, ctx, R):
        from stochopy_amd import _device, _lib, _rng

        t = _device.torch()
        self.ctx, self.L, self.R = ctx, ctx.L, R
        keys = np.array([_rng.philox_key(SEED + r) for r in range(R)], dtype=np.uint32)
        self.dev = dev = {"keys": ctx.upload(keys.view(np.int32)), "lower": ctx.upload(np.full(N, -5.12)),
                          "upper": ctx.upload(np.full(N, 5.12)), "xs": ctx.empty((R, N)), "funs": ctx.empty((R,)),
                          "nits": ctx.empty((R,), dtype=t.int64), "statuses": ctx.empty((R,), dtype=t.int32)}
        self.a = a = _lib.SxDeRunsArgs()
        for name in dev:
            setattr(a, name, _device.ptr(dev[name]))
        a.R, a.P, a.x0_stride, a.n = R, P, 0, N
        a.fun_id, a.strategy, a.constraints, a.maxiter = _lib.FUN_IDS["rosenbrock"], _lib.DE_STRATEGIES["best1bin"], 0, MAXITER
        a.F, a.CR, a.xtol, a.ftol = 0.5, 0.9, OPTS["xtol"], OPTS["ftol"]
        self.evals = R * MAXITER * P

    def timed(self, launches=1):
        """Seconds per launch (a whole batch), over `launches` launches back to back."""
        from stochopy_amd import _lib

        t = __import__("torch")
        with t.cuda.stream(self.ctx.stream):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                _lib.check(self.L.sx_de_runs_launch(C.byref(self.a), self.ctx.stream_ptr), "sx_de_runs_launch")
            e1.record()
            e1.synchronize()
        assert int(self.dev["nits"].min()) == MAXITER  # every run did all its generations
        return e0.elapsed_time(e1) * 1e-3 / launches


def whole_call(sa, R):
    """Wall seconds of one minimize(..., runs=R) call."""
    t0 = time.perf_counter()
    res = sa.optimize.minimize(sa.factory.rosenbrock, BOUNDS, method="de", options=dict(OPTS, seed=SEED, runs=R))
    dt = time.perf_counter() - t0
    assert res.nfev == R * MAXITER * P
    return dt


def loop_of_calls(sa, ctx, calls):
    """Wall seconds per call of `calls` single minimize() calls, one after the other."""
    t0 = time.perf_counter()
    for r in range(calls):
        res = sa.optimize.minimize(sa.factory.rosenbrock, BOUNDS, method="de", options=dict(OPTS, seed=SEED + r))
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
    batches = [DeviceBatch(ctx, R) for R in RUNS]
    launches = {}
    for b in batches:
        b.timed()  # warm-up: code object load
        launches[b.R] = max(1, int(round(args.window / b.timed())))
        whole_call(sa, b.R)
    loop_of_calls(sa, ctx, 8)  # warm-up: graphs of the chained kernel, allocator
    times = {b.R: [] for b in batches}
    calls = {b.R: [] for b in batches}
    loop = []
    for _ in range(args.rounds):
        for b in batches:
            times[b.R].append(b.timed(launches[b.R]))
            calls[b.R].append(whole_call(sa, b.R))
        loop.append(loop_of_calls(sa, ctx, args.loop_calls))
    loop = np.array(loop)
    per_call = MAXITER * P
    loop_rate = per_call / float(np.median(loop))
    lines = [{"config": "loop of single minimize() calls", "calls_timed": args.loop_calls, "rounds": args.rounds,
              "seconds_per_call_median": float(np.median(loop)), "seconds_per_call_min": float(loop.min()),
              "seconds_per_call_max": float(loop.max()), "us_per_generation": float(np.median(loop)) / MAXITER * 1e6,
              "evals_per_s": loop_rate, "evals_per_s_spread": [per_call / float(loop.max()), per_call / float(loop.min())]}]
    for b in batches:
        ts, cs = np.array(times[b.R]), np.array(calls[b.R])
        rate = b.evals / float(np.median(ts))
        lines.append({"config": "runs", "runs": b.R, "ndim": N, "popsize": P, "maxiter": MAXITER, "rounds": args.rounds,
                      "launches_per_round": launches[b.R], "seconds_median": float(np.median(ts)),
                      "seconds_min": float(ts.min()), "seconds_max": float(ts.max()), "evals_per_s": rate,
                      "evals_per_s_spread": [b.evals / float(ts.max()), b.evals / float(ts.min())],
                      "call_seconds_median": float(np.median(cs)), "call_evals_per_s": b.evals / float(np.median(cs)),
                      "loop_evals_per_s": loop_rate, "loop_seconds_for_these_runs_at_that_rate": b.R * float(np.median(loop)),
                      "ratio_kernel_to_loop": rate / loop_rate,
                      "ratio_call_to_loop": b.evals / float(np.median(cs)) / loop_rate})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
