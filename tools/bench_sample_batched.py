#!/usr/bin/env python3
"""What a caller's own device objective costs the samplers: stochopy_amd.sample with a factory objective (fused: one resident
launch, csrc/sx_sample.hip) against the same objective handed in as factory.batched (csrc/sx_sample_unfused.hip: per sample
propose -> objective -> decide, hmc with nleap + 2 rounds of gradient -> leap in between), on one MI355X.

The "caller's" objective and gradient are the library's own kernels behind the hook (sx_eval, sx_sample_gradient), so both
sides do the same arithmetic and the difference is the launches and the trips through memory.  Shapes are the README's
sampler shapes: 16 384 chains, rosenbrock, Philox draws, return_all off;
    mcmc  ndim 128, perc 1.0
    hmc   ndim 64, nleap 10, fused jac="analytic" against jac=factory.batched(gradient)
Every configuration is warmed up once, then the configurations take turns for --rounds rounds; a line gives the median and
the spread of its rounds.  Time = host clock around whole sample() calls (repeated back to back for ~--window seconds per
round, divided by their number); a call ends with the results on the host, so the time includes the call's allocations and
copies: what a caller sees.

    python tools/bench_sample_batched.py [--rounds 5] [--chains 16384] [--window 0.25] [--out FILE]
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


def wrappers(sa, name):
    import torch

    from stochopy_amd import _lib

    L, fid = _lib.lib(), _lib.FUN_IDS[name]

    def stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fun(X):
        P, n = X.shape
        f = torch.empty((P,), dtype=torch.float64, device=X.device)
        _lib.check(L.sx_eval(fid, X.data_ptr(), P, n, n, None, None, f.data_ptr(), None, None, stream()), "sx_eval")
        return f

    def grad(X):
        P, n = X.shape
        G = torch.empty((P, n), dtype=torch.float64, device=X.device)
        _lib.check(L.sx_sample_gradient(fid, X.data_ptr(), P, n, G.data_ptr(), stream()), "sx_sample_gradient")
        return G

    return sa.factory.batched(fun), sa.factory.batched(grad)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back calls per timed round")
    ap.add_argument("--out")
    args = ap.parse_args()
    import stochopy_amd as sa

    fun, grad = wrappers(sa, "rosenbrock")
    common = {"seed": 3, "rng": "philox", "chains": args.chains, "return_all": False, "backend": "hip"}
    mcmc = {"stepsize": 0.05, "perc": 1.0}
    hmc = {"nleap": 10, "stepsize": 0.001}
    configs = [
        ("mcmc fused", "mcmc", 128, sa.factory.rosenbrock, dict(mcmc, maxiter=1000)),
        ("mcmc batched", "mcmc", 128, fun, dict(mcmc, maxiter=200)),
        ("hmc fused analytic", "hmc", 64, sa.factory.rosenbrock, dict(hmc, maxiter=100, jac="analytic")),
        ("hmc batched gradient", "hmc", 64, fun, dict(hmc, maxiter=50, jac=grad)),
    ]

    def timed(method, ndim, f, o, calls=1):
        """Seconds per sample() call, over `calls` calls back to back."""
        t0 = time.perf_counter()
        for _ in range(calls):
            sa.sample.sample(f, [[-5.12, 5.12]] * ndim, method=method, options=dict(common, **o))
        return (time.perf_counter() - t0) / calls

    times = {tag: [] for tag, *_ in configs}
    calls = {}
    for tag, method, ndim, f, o in configs:
        timed(method, ndim, f, o)  # warm-up: code object load, allocator
        calls[tag] = max(1, int(round(args.window / timed(method, ndim, f, o))))
    for _ in range(args.rounds):
        for tag, method, ndim, f, o in configs:
            times[tag].append(timed(method, ndim, f, o, calls[tag]))
    lines = []
    for tag, method, ndim, f, o in configs:
        ts = np.array(times[tag])
        samples = args.chains * o["maxiter"]
        lines.append({"config": tag, "method": method, "ndim": ndim, "chains": args.chains, "maxiter": o["maxiter"],
                      "seconds_median": float(np.median(ts)), "seconds_min": float(ts.min()), "seconds_max": float(ts.max()),
                      "samples_per_s": samples / float(np.median(ts)),
                      "samples_per_s_spread": [samples / float(ts.max()), samples / float(ts.min())], "rounds": args.rounds,
                      "calls_per_round": calls[tag]})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as out:
            for line in lines:
                out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
