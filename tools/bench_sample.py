#!/usr/bin/env python3
"""Throughput of the samplers' chain kernels (csrc/sx_sample.hip) on one MI355X, next to the same sampler on one CPU core.

Configurations (chains = 16 384, rosenbrock, Philox draws; xall stays on the device while timed):
    mcmc           ndim 128, maxiter 1000, return_all off
    mcmc+xall      ndim 128, maxiter 200,  return_all on  (xall is 3.4 GB; the bytes stored per second are given as a share
                   of the HBM peak DESIGN.md uses, 8 TB/s -- 14 %: not bound by writing it, see --adapt and DESIGN.md §19)
    hmc analytic   ndim 64,  maxiter 100,  nleap 10, jac="analytic"
    hmc fd         ndim 64,  maxiter 10,   nleap 10, finite differences (1 536 objective calls per sample and chain)
Every configuration is warmed up once, then the configurations take turns for --rounds rounds; the line of a configuration
gives the median and the spread (min .. max) of its rounds.  Time = device events around a round's launches of sx_sample_run
(each a whole run from sample 0, repeated back to back for ~0.25 s), divided by their number.
CPU side: the reference package when it is importable, else its numpy restatement (tests/_sample_oracle.py) -- the same numpy
calls per sample -- with the same settings and ONE chain, on one core.

    python tools/bench_sample.py [--rounds 5] [--chains 16384] [--window 0.25] [--no-cpu] [--out FILE]

--tempered: what parallel tempering costs (csrc/sx_sample_temper.hip).  The `mcmc` configuration above (the plain kernel:
the baseline of the session) takes turns, by the same protocol, with the same --chains replicas as chains / 16 ladders of 16
rungs (temperatures geomspace(1, 64, 16)), exchanging after every sample (swap_every 1) and after every 10th; samples / s
counts every replica's samples, `vs_plain` is the ratio of the medians.  No CPU side.

    python tools/bench_sample.py --tempered [--rounds 5] [--out profiles/sample_temper_bench.jsonl]

--adapt: what the warm-up and thinning cost (sx_sample_run_adapt).  The four configurations above take turns, by the same
protocol, with `mcmc` and `hmc analytic` adapting their step for warmup = maxiter // 2 samples (`vs_plain`: samples / s over the
plain configuration's, ratio of the medians) and with `mcmc+xall` keeping every 10th sample (thin=10: a tenth of the bytes;
its line carries the bytes stored per second and `vs_plain` too).

    python tools/bench_sample.py --adapt --no-cpu [--rounds 5] [--out FILE]

--metric: what the per-axis scales cost (sx_sample_run_metric, metric="diag").  `mcmc` and `hmc analytic`, plain, with
warmup = maxiter // 2 alone and with the scales learnt in the windows of that warm-up, take turns by the same protocol.  The
metric line carries `vs_warmup` (samples / s over the whole call, over the warm-up-only line's), the chains per workgroup of
either form, and `sampling_vs_warmup`: the same ratio over the sampling phase alone -- each form's whole run minus a run that
stops after its warm-up (maxiter = warmup + 1), timed the same way.

    python tools/bench_sample.py --metric --no-cpu [--rounds 5] [--out profiles/sample_metric_bench.jsonl]

--ensemble: the affine-invariant ensemble sampler (csrc/sx_sample_ensemble.hip, method="ensemble"): rosenbrock, return_all off,
maxiter 300, ndim 32 with 256 ensembles of 64 walkers and ndim 64 with 128 ensembles of 128 walkers, each taking turns by the same
protocol with the plain mcmc kernel (perc 1.0) on as many chains as there are walkers at the same ndim.  samples / s counts every
walker's samples; `vs_plain` is the ratio of the medians.  --chains is not used.  No CPU side.

    python tools/bench_sample.py --ensemble [--rounds 5] [--out profiles/sample_ensemble_bench.jsonl]

--ensemble --moves: the moves of the ensemble sampler (csrc/sx_sample_ensemble_moves.hip) at the same two shapes: "de", "snooker"
and the mixture [("de", .7), ("de", .1, 1.0), ("snooker", .2)] through sx_sample_ensemble_run_moves, each taking turns by the same
protocol with the stretch move through sx_sample_ensemble_run; `vs_stretch` is the ratio of the medians.

    python tools/bench_sample.py --ensemble --moves [--rounds 5] [--out profiles/sample_ensemble_moves_bench.jsonl]

--smc: tempered sequential Monte Carlo (csrc/sx_sample_smc.hip, method="smc"): rosenbrock, 16 populations of 1 024 particles at
ndim 4 and ndim 128.  The mutation launch (sx_smc_mutate of stage 1, 200 steps per particle, after one init / stage / resample)
takes turns by the same protocol with the plain mcmc kernel (perc 1.0, 201 samples, return_all off) on as many chains at the
same ndim; samples / s counts every particle's steps, `vs_mcmc` is the ratio of the medians.  Then the whole run of the public
call on the sphere of tests/_smc_cases.py (16 x 1 024 particles, 8 steps, ndim 4): wall-clock seconds over --rounds runs, and
the stages.  --chains is not used.  No CPU side.

    python tools/bench_sample.py --smc [--rounds 5] [--out profiles/sample_smc_bench.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12  # bytes/s, as in DESIGN.md

CONFIGS = [
    ("mcmc", "mcmc", 128, {"maxiter": 1000, "stepsize": 0.05, "perc": 1.0, "return_all": False}),
    ("mcmc+xall", "mcmc", 128, {"maxiter": 200, "stepsize": 0.05, "perc": 1.0, "return_all": True}),
    ("hmc analytic", "hmc", 64, {"maxiter": 100, "nleap": 10, "stepsize": 0.001, "jac": "analytic", "return_all": False}),
    ("hmc fd", "hmc", 64, {"maxiter": 10, "nleap": 10, "stepsize": 0.001, "jac": None, "return_all": False}),
]


class DeviceRun:
    """The buffers and arguments of one configuration, launched as stochopy_amd.sample does without a callback."""

    def __init__(self, ctx, method, ndim, chains, o, seed=3):
        from stochopy_amd import _lib
        from stochopy_amd.sample._chains import chain_args

        self.ctx, self.L, self.m = ctx, ctx.L, o["maxiter"]
        lower, upper = np.full(ndim, -5.12), np.full(ndim, 5.12)
        s = types.SimpleNamespace(  # the fields of sample._chains.Setup that chain_args reads
            chains=chains, ndim=ndim, maxiter=self.m, lower=lower, upper=upper,
            step=np.full(ndim, o["stepsize"]) * (0.5 * (upper - lower)), fun_id=_lib.FUN_IDS["rosenbrock"],
            method=_lib.SX_SAMPLE_MCMC if method == "mcmc" else _lib.SX_SAMPLE_HMC, reject=False,
            k=max(1, int(o.get("perc", 1.0) * ndim)), nleap=o.get("nleap", 1),
            jac=_lib.SX_JAC_ANALYTIC if o.get("jac") == "analytic" else _lib.SX_JAC_FINITE_DIFF, fd_step=1.0e-4, key=(seed, 0))
        self.dev, self.a = chain_args(ctx, s, self.m if o["return_all"] else None)
        self.samples = chains * self.m
        self.stored = chains * self.m * (ndim + 1) * 8 if o["return_all"] else 0

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_sample_run(C.byref(self.a), 0, self.m, self.ctx.stream_ptr), "sx_sample_run")

    def timed(self, launches=1):
        """Seconds per launch (a whole run from sample 0), over `launches` launches back to back."""
        t = __import__("torch")
        with t.cuda.stream(self.ctx.stream):
            e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                self.launch()
            e1.record()
            e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / launches


class TemperedRun(DeviceRun):
    """The same replicas as ladders of K rungs, launched as stochopy_amd.sample does with temperatures=..."""

    def __init__(self, ctx, ndim, replicas, K, swap_every, o):
        from stochopy_amd import _device

        super().__init__(ctx, "mcmc", ndim, replicas, o)
        t = _device.torch()
        self.K, self.swap_every = K, swap_every
        self.beta = ctx.upload(1.0 / np.geomspace(1.0, 64.0, K))
        self.nswap = ctx.zeros((replicas,), dtype=t.int64)

    def launch(self):
        from stochopy_amd import _device, _lib

        _lib.check(self.L.sx_sample_tempered_run(C.byref(self.a), _device.ptr(self.beta), self.K, self.swap_every,
                                                 _device.ptr(self.nswap), 0, self.m, self.ctx.stream_ptr),
                   "sx_sample_tempered_run")


class EnsembleRun(DeviceRun):
    """`ensembles` ensembles of W walkers, launched as stochopy_amd.sample does with method="ensemble"."""

    def __init__(self, ctx, ndim, ensembles, W, o, stretch=2.0):
        from stochopy_amd import _lib

        super().__init__(ctx, "mcmc", ndim, ensembles * W, o)
        self.a.method = _lib.SX_SAMPLE_ENSEMBLE
        self.W, self.stretch = W, stretch
        self.lds = ctx.L.sx_sample_ensemble_lds_bytes(W, ndim)

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_sample_ensemble_run(C.byref(self.a), self.W, self.stretch, 0, self.m, self.ctx.stream_ptr),
                   "sx_sample_ensemble_run")


class EnsembleMovesRun(EnsembleRun):
    """The same ensembles with ``moves``, launched as stochopy_amd.sample does with method="ensemble" and moves=..."""

    def __init__(self, ctx, ndim, ensembles, W, o, moves):
        from stochopy_amd import _lib
        from stochopy_amd.sample import _ensemble

        super().__init__(ctx, ndim, ensembles, W, o)
        self.moves, cum = _ensemble.check_moves(moves, ndim, W, self.stretch)
        self.mv = mv = _lib.SxSampleEnsembleOpts()
        mv.nmoves = len(self.moves)
        for k, (name, _, param) in enumerate(self.moves):
            mv.kind[k], mv.cum[k], mv.param[k] = _ensemble.MOVE_KINDS[name], cum[k], param
        mv.rec_start, mv.rec_every, mv.rec_rows = 0, 1, self.m

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_sample_ensemble_run_moves(C.byref(self.a), self.W, C.byref(self.mv), 0, self.m, self.ctx.stream_ptr),
                   "sx_sample_ensemble_run_moves")


ENSEMBLE_MOVES = {"de": "de", "snooker": "snooker", "mixture": [("de", 0.7), ("de", 0.1, 1.0), ("snooker", 0.2)]}
ENSEMBLE_SHAPES = [(32, 64, 256), (64, 128, 128)]  # (ndim, walkers, ensembles)
ENSEMBLE_OPTIONS = {"maxiter": 300, "stepsize": 0.05, "perc": 1.0, "return_all": False}


class SmcMutateRun:
    """The mutation launch of stage 1 of `populations` populations of P particles, M steps per particle, as stochopy_amd.sample
    launches it with method="smc" (after the init, stage and resample launches, which are not timed)."""

    stored = 0
    timed = DeviceRun.timed

    def __init__(self, ctx, ndim, populations, P, M, seed=3):
        from stochopy_amd import _lib
        from stochopy_amd.sample import _smc

        self.ctx, self.L, self.m, self.samples = ctx, ctx.L, M, populations * P * M
        s = types.SimpleNamespace(chains=populations, particles=P, ndim=ndim, lower=np.full(ndim, -5.12), upper=np.full(ndim, 5.12),
                                  fun_id=_lib.FUN_IDS["rosenbrock"], steps=M, maxiter=2, ess=0.5, target=0.234,
                                  scale=2.38 / np.sqrt(ndim), key=(seed, 0))
        t = __import__("torch")
        with t.cuda.stream(ctx.stream):
            self.dev, self.a = _smc.smc_args(ctx, s)
            _lib.check(self.L.sx_smc_init(C.byref(self.a), ctx.stream_ptr), "sx_smc_init")
            _lib.check(self.L.sx_smc_stage(C.byref(self.a), 1, ctx.stream_ptr), "sx_smc_stage")
            _lib.check(self.L.sx_smc_resample(C.byref(self.a), 1, ctx.stream_ptr), "sx_smc_resample")
        ctx.sync()

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_smc_mutate(C.byref(self.a), 1, self.ctx.stream_ptr), "sx_smc_mutate")


SMC_SHAPES = [(4, 16, 1024), (128, 16, 1024)]  # (ndim, populations, particles)
SMC_STEPS = 200


def smc_whole_run(rounds):
    """The public call on the sphere of tests/_smc_cases.py: wall-clock seconds per run."""
    import _smc_cases as cases
    import stochopy_amd as sa

    def once():
        t0 = time.perf_counter()
        res = sa.sample.sample(sa.factory.sphere, cases.SPHERE_BOUNDS, method="smc", options=dict(cases.SPHERE_OPTIONS, seed=1))
        return time.perf_counter() - t0, res

    once()
    ts, res = [], None
    for _ in range(rounds):
        dt, res = once()
        ts.append(dt)
    o = cases.SPHERE_OPTIONS
    return {"config": "smc whole run, sphere ndim=4", "method": "smc", "ndim": 4, "populations": o["chains"],
            "particles": o["particles"], "steps": o["steps"], "stages": int(res.nit), "nfev": int(res.nfev),
            "seconds_median": float(np.median(ts)), "seconds_min": float(min(ts)), "seconds_max": float(max(ts)),
            "particle_steps_per_s": o["chains"] * o["particles"] * o["steps"] * int(res.nit) / float(np.median(ts)), "rounds": rounds}


class AdaptRun(DeviceRun):
    """The same configuration through sx_sample_run_adapt, as stochopy_amd.sample launches it with warmup / burn / thin."""

    def __init__(self, ctx, method, ndim, chains, o, warmup=0, burn=0, thin=1):
        from stochopy_amd import _device, _lib

        t = _device.torch()
        rows = -(-(o["maxiter"] - burn) // thin)
        self.rows = rows
        super().__init__(ctx, method, ndim, chains, o)
        if o["return_all"]:  # (the parent's (chains, maxiter, ndim) arrays are dropped for the thinned ones)
            self.dev["xall"], self.dev["funall"] = ctx.empty((chains, rows, ndim)), ctx.empty((chains, rows))
            self.a.xall, self.a.funall = _device.ptr(self.dev["xall"]), _device.ptr(self.dev["funall"])
            self.stored = chains * rows * (ndim + 1) * 8
        self.ad = ad = _lib.SxSampleAdapt()
        if warmup > 0:
            self.state = {name: ctx.empty((chains,)) for name in ("scale", "hbar", "logsbar")}
            self.state["nacc_warm"] = ctx.empty((chains,), dtype=t.int64)
            for name, buf in self.state.items():
                setattr(ad, name, _device.ptr(buf))
        ad.warmup, ad.rec_start, ad.rec_every, ad.rec_rows = warmup, burn, thin, rows
        ad.target = 0.234 if method == "mcmc" else 0.65

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_sample_run_adapt(C.byref(self.a), C.byref(self.ad), 0, self.m, self.ctx.stream_ptr),
                   "sx_sample_run_adapt")


class MetricRun(AdaptRun):
    """The same configuration through sx_sample_run_metric, as stochopy_amd.sample launches it with metric="diag"."""

    def __init__(self, ctx, method, ndim, chains, o, warmup):
        from stochopy_amd.sample import _adapt
        from stochopy_amd.sample._chains import metric_args

        super().__init__(ctx, method, ndim, chains, o, warmup=warmup, burn=min(warmup, o["maxiter"] - 1))
        self.mt = metric_args(ctx, self.dev, chains, ndim, *_adapt.metric_windows(warmup))

    def launch(self):
        from stochopy_amd import _lib

        _lib.check(self.L.sx_sample_run_metric(C.byref(self.a), C.byref(self.ad), C.byref(self.mt), 0, self.m,
                                               self.ctx.stream_ptr), "sx_sample_run_metric")


def metric_chains_per_workgroup(method, jac, ndim):
    """Chains per workgroup of the form with per-axis scales: csrc/sx_sample.hpp sample_waves with the row that holds eff --
    the largest power of two of waves (<= 8 waves, <= 16 chains) whose rows fit 64 KiB."""
    lpr = 16 if ndim <= 64 else 32 if ndim <= 128 else 64
    stride = ndim + 8  # (gen_row_stride for ndim <= 256, the benchmark's range)
    row = {"mcmc": ndim + stride, "analytic": 2 * ndim + stride, None: 2 * ndim + 3 * stride}[method if method == "mcmc" else jac]
    row = (row + ndim) * 8
    rpw, w = 64 // lpr, 1
    while 2 * w <= 8 and 2 * w * rpw <= 16 and 2 * w * rpw * row <= 64 * 1024:
        w *= 2
    return w * rpw


def cpu_rate(method, ndim, o):
    """Samples per second of one chain on one core, and what ran."""
    o = dict(o, seed=3)
    o["maxiter"] = {"mcmc": 2000, "hmc": 100 if o.get("jac") == "analytic" else 8}[method]
    bounds = [[-5.12, 5.12]] * ndim
    try:
        np.Inf = np.inf
        from stochopy import factory
        from stochopy.sample import sample

        if o.get("jac") == "analytic":
            raise ImportError  # (the reference has no working jac: its numbers are the finite-difference ones)
        what, call = "reference", lambda: sample(factory.rosenbrock, bounds, method=method, options=o)
    except ImportError:
        import _sample_oracle

        what = "numpy restatement"
        call = lambda: _sample_oracle.sample("rosenbrock", bounds, method=method, options=dict(o, rng="numpy-legacy"))  # noqa: E731
    with np.errstate(all="ignore"):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
    return o["maxiter"] / dt, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of back-to-back launches per timed round")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--tempered", action="store_true", help="the plain mcmc kernel next to ladders of 16 replicas")
    ap.add_argument("--adapt", action="store_true", help="the plain configurations next to a warm-up and to thin=10")
    ap.add_argument("--metric", action="store_true", help="plain, warm-up alone and warm-up with per-axis scales")
    ap.add_argument("--ensemble", action="store_true", help="the ensemble sampler next to the plain mcmc kernel on as many rows")
    ap.add_argument("--moves", action="store_true", help='with --ensemble: "de", "snooker" and their mixture next to the stretch move')
    ap.add_argument("--smc", action="store_true", help="the mutation launch of method=\"smc\" next to the plain mcmc kernel; the whole run")
    args = ap.parse_args()
    if args.moves and not args.ensemble:
        ap.error("--moves goes with --ensemble")
    from stochopy_amd import _device

    ctx = _device.Context()
    ensemble_of, stretch_of, mcmc_of = {}, {}, {}
    if args.smc:
        args.no_cpu = True
        runs = []
        for ndim, populations, P in SMC_SHAPES:
            o = {"maxiter": SMC_STEPS + 1, "stepsize": 0.05, "perc": 1.0, "return_all": False}
            plain, tag = f"mcmc ndim={ndim} chains={populations * P}", f"smc mutation ndim={ndim} populations={populations} particles={P}"
            runs.append((plain, "mcmc", ndim, o, DeviceRun(ctx, "mcmc", ndim, populations * P, o)))
            runs.append((tag, "smc", ndim, {"maxiter": SMC_STEPS, "populations": populations, "particles": P},
                         SmcMutateRun(ctx, ndim, populations, P, SMC_STEPS)))
            mcmc_of[tag] = plain
    elif args.ensemble and args.moves:
        args.no_cpu = True
        runs, o = [], ENSEMBLE_OPTIONS
        for ndim, W, ensembles in ENSEMBLE_SHAPES:
            shape = f"ndim={ndim} W={W} ensembles={ensembles}"
            runs.append((f"ensemble {shape}", "ensemble", ndim, dict(o, walkers=W, ensembles=ensembles, stretch=2.0),
                         EnsembleRun(ctx, ndim, ensembles, W, o)))
            for name, moves in ENSEMBLE_MOVES.items():
                run = EnsembleMovesRun(ctx, ndim, ensembles, W, o, moves)
                runs.append((f"ensemble moves={name} {shape}", "ensemble", ndim,
                             dict(o, walkers=W, ensembles=ensembles, moves=[list(e) for e in run.moves]), run))
                stretch_of[runs[-1][0]] = f"ensemble {shape}"
    elif args.ensemble:
        args.no_cpu = True
        runs, o = [], ENSEMBLE_OPTIONS
        for ndim, W, ensembles in ENSEMBLE_SHAPES:
            plain, tag = f"mcmc ndim={ndim} chains={ensembles * W}", f"ensemble ndim={ndim} W={W} ensembles={ensembles}"
            runs.append((plain, "mcmc", ndim, o, DeviceRun(ctx, "mcmc", ndim, ensembles * W, o)))
            runs.append((tag, "ensemble", ndim, dict(o, walkers=W, ensembles=ensembles, stretch=2.0),
                         EnsembleRun(ctx, ndim, ensembles, W, o)))
            ensemble_of[tag] = plain
    elif args.tempered:
        args.no_cpu = True
        tag, method, ndim, o = CONFIGS[0]
        runs = [(tag, method, ndim, o, DeviceRun(ctx, method, ndim, args.chains, o))]
        for every in (1, 10):
            runs.append((f"tempered K=16 swap_every={every}", method, ndim, dict(o, ladders=args.chains // 16, K=16, swap_every=every),
                         TemperedRun(ctx, ndim, args.chains // 16 * 16, 16, every, o)))
    else:
        runs = [(tag, method, ndim, o, DeviceRun(ctx, method, ndim, args.chains, o)) for tag, method, ndim, o in CONFIGS]
    plain_of = {}
    if args.adapt:
        by_tag = {tag: (method, ndim, o) for tag, method, ndim, o in CONFIGS}
        for tag in ("mcmc", "hmc analytic"):
            method, ndim, o = by_tag[tag]
            W = o["maxiter"] // 2
            new = f"{tag} warmup={W}"
            runs.append((new, method, ndim, dict(o, warmup=W), AdaptRun(ctx, method, ndim, args.chains, o, warmup=W, burn=W)))
            plain_of[new] = tag
        method, ndim, o = by_tag["mcmc+xall"]
        runs.append(("mcmc+xall thin=10", method, ndim, dict(o, thin=10), AdaptRun(ctx, method, ndim, args.chains, o, thin=10)))
        plain_of["mcmc+xall thin=10"] = "mcmc+xall"
    warm_of, short_of = {}, {}
    if args.metric:
        from stochopy_amd import _lib

        args.no_cpu = True
        by_tag = {tag: (method, ndim, o) for tag, method, ndim, o in CONFIGS}
        runs = [r for r in runs if r[0] in ("mcmc", "hmc analytic")]
        for tag in ("mcmc", "hmc analytic"):
            method, ndim, o = by_tag[tag]
            W = o["maxiter"] // 2
            short = dict(o, maxiter=W + 1)  # the run that stops after its warm-up: what the sampling phase is measured against
            for kind in ("warmup", "warmup+metric"):
                for which, oo in (("", o), (" (warm-up only)", short)):
                    if kind == "warmup":
                        run = AdaptRun(ctx, method, ndim, args.chains, oo, warmup=W, burn=min(W, oo["maxiter"] - 1))
                    else:
                        run = MetricRun(ctx, method, ndim, args.chains, oo, warmup=W)
                    runs.append((f"{tag} {kind}={W}{which}", method, ndim, dict(oo, warmup=W), run))
                    plain_of[f"{tag} {kind}={W}{which}"] = tag
            warm_of[f"{tag} warmup+metric={W}"] = f"{tag} warmup={W}"
            for kind in ("warmup", "warmup+metric"):
                short_of[f"{tag} {kind}={W}"] = f"{tag} {kind}={W} (warm-up only)"
            jac = _lib.SX_JAC_ANALYTIC if o.get("jac") == "analytic" else _lib.SX_JAC_FINITE_DIFF
            meth = _lib.SX_SAMPLE_MCMC if method == "mcmc" else _lib.SX_SAMPLE_HMC
            print(json.dumps({"config": tag, "ndim": ndim,
                              "chains_per_workgroup": ctx.L.sx_sample_chains_per_workgroup(meth, jac, ndim),
                              "chains_per_workgroup_metric": metric_chains_per_workgroup(method, o.get("jac"), ndim)}), flush=True)
    launches = {}
    for tag, *_, r in runs:
        r.timed()  # warm-up: code object load, first touch of xall
        launches[tag] = max(1, int(round(args.window / r.timed())))  # a timed window of ~args.window seconds
    times = {tag: [] for tag, *_ in runs}
    for _ in range(args.rounds):
        for tag, *_, r in runs:
            times[tag].append(r.timed(launches[tag]))
    lines = []
    runs_maxiter = {tag: o["maxiter"] for tag, _, _, o, _ in runs}
    runs_rate = {tag: r.samples / float(np.median(times[tag])) for tag, *_, r in runs}
    for tag, method, ndim, o, r in runs:
        ts = np.array(times[tag])
        line = {"config": tag, "method": method, "ndim": ndim, "chains": r.samples // r.m, "maxiter": o["maxiter"],
                "seconds_median": float(np.median(ts)), "seconds_min": float(ts.min()), "seconds_max": float(ts.max()),
                "samples_per_s": r.samples / float(np.median(ts)),
                "samples_per_s_spread": [r.samples / float(ts.max()), r.samples / float(ts.min())], "rounds": args.rounds, "launches_per_round": launches[tag]}
        if args.tempered:
            line.update({k: o[k] for k in ("ladders", "K", "swap_every") if k in o})
            line["vs_plain"] = float(np.median(times[runs[0][0]])) / float(np.median(ts)) * r.samples / runs[0][4].samples
        if tag in ensemble_of:
            line.update({k: o[k] for k in ("walkers", "ensembles", "stretch")})
            line["lds_bytes"] = r.lds
            line["vs_plain"] = float(np.median(times[ensemble_of[tag]])) / float(np.median(ts))
        if tag in mcmc_of:
            line.update({k: o[k] for k in ("populations", "particles")})
            line["vs_mcmc"] = line["samples_per_s"] / (runs_rate[mcmc_of[tag]])
        if tag in stretch_of:
            line.update({k: o[k] for k in ("walkers", "ensembles", "moves")})
            line["lds_bytes"] = r.lds
            line["vs_stretch"] = float(np.median(times[stretch_of[tag]])) / float(np.median(ts))
        if tag in plain_of:
            line.update({k: o[k] for k in ("warmup", "thin") if k in o})
            line["vs_plain"] = float(np.median(times[plain_of[tag]])) / float(np.median(ts)) * o["maxiter"] / runs_maxiter[plain_of[tag]]
        if tag in warm_of:
            med = {t: float(np.median(times[t])) for t in times}
            line["vs_warmup"] = med[warm_of[tag]] / med[tag]
            line["sampling_vs_warmup"] = (med[warm_of[tag]] - med[short_of[warm_of[tag]]]) / (med[tag] - med[short_of[tag]])
        if r.stored:
            line["stored_bytes_per_s"] = r.stored / float(np.median(ts))
            line["share_of_hbm_peak"] = line["stored_bytes_per_s"] / HBM_PEAK
        if not args.no_cpu:
            rate, what = cpu_rate(method, ndim, o)
            line.update({"cpu_one_chain_samples_per_s": rate, "cpu_what": what, "speedup": line["samples_per_s"] / rate})
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.smc:
        lines.append(smc_whole_run(args.rounds))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
