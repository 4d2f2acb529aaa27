#!/usr/bin/env python3
"""Throughput of many independent VD-CMA runs in one launch (options["runs"], csrc/sx_vd_runs.hip) on one MI355X, next to the
only way to do the same work without it: a Python loop of single minimize() calls.

Workload: rosenbrock, maxiter = 200, xtol = 0 and ftol = -1 (rules 0 and 1 never trigger), Philox draws; every run must do its
200 generations (checked); two shapes: n = 64, popsize = 16 (the reference's default population 4 + 3 ln n) and n = 256,
popsize = 20.
    runs R in {256, 4096, 16384}   ONE sx_vd_runs_launch of R workgroups; time = device events around a round's launches
                                   (each a whole batch from the first generation, repeated back to back for ~--window seconds),
                                   divided by their number.  "call" is the wall time of one whole minimize(..., runs=R) call on
                                   top: the R initial means and directions drawn on the host, uploads, launch, results back.
    loop                           --loop-calls (64) single minimize(method="vdcma", rng="philox") calls with the same settings
                                   and seeds s, s+1, ..., wall time with the stream drained at the end.  The loop's rate does
                                   not depend on how many runs are asked for: the figure beside R runs IS this rate, not a
                                   measurement of R calls.
Everything is warmed up once, then the configurations take turns for --rounds rounds; a line gives the median and the spread
(min .. max) of its rounds, in objective evaluations per second (nit x popsize per run).

    python tools/bench_vd_runs.py [--rounds 5] [--window 0.25] [--loop-calls 64] [--out FILE]
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

MAXITER, SEED, SIGMA, MUPERC = 200, 3, 0.1, 0.5
SHAPES = ((64, 16), (256, 20))  # (ndim, popsize)
RUNS = (256, 4096, 16384)
OPTS = {"maxiter": MAXITER, "sigma": SIGMA, "xtol": 0.0, "ftol": -1.0, "rng": "philox", "backend": "hip"}
HALF = 3.0


class DeviceBatch:
    """The buffers and arguments of one batch, launched as optimize.minimize(..., runs=R) does."""

    def __init__(self, ctx, n, P, R):
        from stochopy_amd import _device, _lib, _rng
        from stochopy_amd.optimize._vdcma import _strategy_constants

        t = _device.torch()
        self.ctx, self.L, self.R, self.n, self.P = ctx, ctx.L, R, n, P
        mu, w, *constants = _strategy_constants(n, P, MUPERC)
        keys = np.array([_rng.philox_key(SEED + r) for r in range(R)], dtype=np.uint32)
        xmean0, vvec0 = np.empty((R, n)), np.empty((R, n))
        for r in range(R):  # (what the single run of seed SEED + r draws: the mean, then the direction)
            init = np.random.RandomState(SEED + r)
            xmean0[r] = init.uniform(-1.0, 1.0, n)
            vvec0[r] = init.randn(n) / np.sqrt(n)
        work = int(ctx.L.sx_vd_runs_workspace_bytes(R, MAXITER)) // 8
        self.dev = dev = {"keys": ctx.upload(keys.view(np.int32)), "xmean0": ctx.upload(xmean0), "vvec0": ctx.upload(vvec0),
                          "xm": ctx.upload(np.zeros(n)),
                          "xstd": ctx.upload(np.full(n, HALF)), "w": ctx.upload(w), "work": ctx.empty((work,)),
                          "xs": ctx.empty((R, n)), "funs": ctx.empty((R,)), "nits": ctx.empty((R,), dtype=t.int64),
                          "statuses": ctx.empty((R,), dtype=t.int32)}
        self.a = a = _lib.SxVdRunsArgs()
        for name in dev:
            setattr(a, name, _device.ptr(dev[name]))
        a.nfevs = a.sigmas = a.xmeans = a.dvecs = a.vvecs = None
        a.R, a.P, a.n, a.mu, a.fun_id, a.maxiter = R, P, n, mu, _lib.FUN_IDS["rosenbrock"], MAXITER
        a.ilim = int(10.0 + 30.0 * n / P)
        a.mueff, a.cc, a.c1, a.cmu = constants
        a.cs, a.ds, a.wsum = 0.3, float(np.sqrt(n)), float(w.sum())
        a.sigma = a.insigma = SIGMA
        a.xtol, a.ftol = OPTS["xtol"], OPTS["ftol"]

    def timed(self, launches=1):
        """Seconds per launch (a whole batch), over `launches` launches back to back; the evaluations one launch did."""
        from stochopy_amd import _lib

        t = __import__("torch")
        with t.cuda.stream(self.ctx.stream):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                _lib.check(self.L.sx_vd_runs_launch(C.byref(self.a), self.ctx.stream_ptr), "sx_vd_runs_launch")
            e1.record()
            e1.synchronize()
        self.evals = int(self.dev["nits"].sum()) * self.P
        self.full = float((self.dev["nits"] == MAXITER).double().mean())
        assert self.full == 1.0, "a run ended before its %d generations" % MAXITER
        return e0.elapsed_time(e1) * 1e-3 / launches


def whole_call(sa, n, P, R):
    """Wall seconds of one minimize(..., runs=R) call."""
    t0 = time.perf_counter()
    res = sa.optimize.minimize(sa.factory.rosenbrock, [[-HALF, HALF]] * n, method="vdcma",
                               options=dict(OPTS, popsize=P, seed=SEED, runs=R))
    dt = time.perf_counter() - t0
    assert res.nfev == int(res.nits.sum()) * P == R * MAXITER * P
    return dt


def loop_of_calls(sa, ctx, n, P, calls):
    """Wall seconds and evaluations of `calls` single minimize() calls, one after the other."""
    t0 = time.perf_counter()
    evals = 0
    for r in range(calls):
        res = sa.optimize.minimize(sa.factory.rosenbrock, [[-HALF, HALF]] * n, method="vdcma",
                                   options=dict(OPTS, popsize=P, seed=SEED + r))
        assert res.nit == MAXITER
        evals += res.nfev
    ctx.sync()
    return time.perf_counter() - t0, evals


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
    batches = [DeviceBatch(ctx, n, P, R) for n, P in SHAPES for R in RUNS]
    launches = {}
    for b in batches:
        b.timed()  # warm-up: code object load
        launches[b] = max(1, int(round(args.window / b.timed())))
        whole_call(sa, b.n, b.P, b.R)
    for n, P in SHAPES:
        loop_of_calls(sa, ctx, n, P, 4)  # warm-up: allocator, code objects of the single run
    times, calls = {b: [] for b in batches}, {b: [] for b in batches}
    loop = {shape: [] for shape in SHAPES}
    for _ in range(args.rounds):
        for b in batches:
            times[b].append(b.timed(launches[b]))
            calls[b].append(whole_call(sa, b.n, b.P, b.R))
        for n, P in SHAPES:
            loop[(n, P)].append(loop_of_calls(sa, ctx, n, P, args.loop_calls))
    lines, loop_rate = [], {}
    for n, P in SHAPES:
        secs = np.array([s for s, _ in loop[(n, P)]])
        rates = np.array([e / s for s, e in loop[(n, P)]])
        gens = np.array([e / P for _, e in loop[(n, P)]])
        loop_rate[(n, P)] = float(np.median(rates))
        lines.append({"config": "loop of single minimize() calls", "method": "vdcma", "ndim": n, "popsize": P,
                      "calls_timed": args.loop_calls, "rounds": args.rounds,
                      "seconds_per_call_median": float(np.median(secs)) / args.loop_calls,
                      "us_per_generation": float(np.median(secs / gens)) * 1e6, "evals_per_s": loop_rate[(n, P)],
                      "evals_per_s_spread": [float(rates.min()), float(rates.max())]})
    for b in batches:
        ts, cs = np.array(times[b]), np.array(calls[b])
        rate, lr = b.evals / float(np.median(ts)), loop_rate[(b.n, b.P)]
        lines.append({"config": "runs", "method": "vdcma", "runs": b.R, "ndim": b.n, "popsize": b.P, "maxiter": MAXITER,
                      "rounds": args.rounds, "launches_per_round": launches[b], "runs_that_did_all_generations": b.full,
                      "evals_per_launch": b.evals, "seconds_median": float(np.median(ts)), "seconds_min": float(ts.min()),
                      "seconds_max": float(ts.max()), "evals_per_s": rate,
                      "evals_per_s_spread": [b.evals / float(ts.max()), b.evals / float(ts.min())],
                      "call_seconds_median": float(np.median(cs)), "call_evals_per_s": b.evals / float(np.median(cs)),
                      "loop_evals_per_s": lr, "loop_seconds_for_these_runs_at_that_rate": b.evals / lr,
                      "ratio_kernel_to_loop": rate / lr, "ratio_call_to_loop": b.evals / float(np.median(cs)) / lr})
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
