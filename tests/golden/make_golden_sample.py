#!/usr/bin/env python3
"""Generate the samplers' golden vectors by RUNNING the reference (stochopy/sample) on the CPU.

Like make_golden.py this script imports keurfonluu/stochopy from a read-only checkout (the directory the environment
variable STOCHOPY_REFERENCE names, present in the build container only) and writes *data* only: tests/golden/sample.json (settings, scalars, callback records, what
numpy's global stream yields next) and tests/golden/sample_xall.npz (xall / funall of every case).

Usage (build container only):
    STOCHOPY_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sample.py

Reference entry points exercised:
    stochopy/sample/_helpers.py:41         sample()
    stochopy/sample/mcmc/_mcmc.py:13       mcmc.sample
    stochopy/sample/hmc/_hmc.py:13         hmc.sample
    stochopy/factory/benchmark.py:14-156   the objectives
"""
import json
import os
import sys

import numpy as np

np.Inf = np.inf  # the reference's samplers still spell it that way

REF = os.environ.get("STOCHOPY_REFERENCE")
if not REF:
    sys.exit("set STOCHOPY_REFERENCE to a checkout of keurfonluu/stochopy")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)

from stochopy import factory  # noqa: E402  (the reference)
from stochopy.sample import sample  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NDIM, BOUND = 8, 5.12
ALL = ["ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang"]
HMC = ["sphere", "rastrigin", "ackley", "griewank", "styblinski_tang"]  # rosenbrock / quartic overflow with these settings


def hx(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 0:
        return float(a).hex()
    return [hx(v) for v in a]


def run(tag, objective, method, options, x0=None, with_callback=False):
    records = []

    def cb(xk, state):
        records.append({"nit": int(state.nit), "fun": hx(state.fun), "accept_ratio": hx(state.accept_ratio),
                        "x": hx(state.x), "xk": hx(xk), "len_xall": len(state.xall), "len_funall": len(state.funall)})

    with np.errstate(all="ignore"):
        res = sample(getattr(factory, objective), [[-BOUND, BOUND]] * NDIM, x0=None if x0 is None else np.array(x0),
                     method=method, options=dict(options), callback=cb if with_callback else None)
    case = {"tag": tag, "objective": objective, "method": method, "ndim": NDIM, "bounds": [-BOUND, BOUND],
            "options": options, "x0": None if x0 is None else hx(x0),
            "result": {"x": hx(res.x), "fun": hx(res.fun), "nit": int(res.nit), "accept_ratio": hx(res.accept_ratio)},
            "next_draws": hx(np.random.rand(4))}
    if method == "hmc":
        case["result"]["nfev"] = int(res.nfev)
    if with_callback:
        case["callback"] = records
    return case, np.array(res.xall), np.array(res.funall)


def main():
    cases, arrays = [], {}
    x0 = np.linspace(-2.0, 3.0, NDIM)
    jobs = []
    for k, name in enumerate(ALL):
        for perc in (1.0, 0.5):
            jobs.append((f"mcmc_{name}_p{int(perc * 100)}", name, "mcmc",
                         {"maxiter": 1000, "stepsize": 0.05, "perc": perc, "seed": 100 + k}, None, False))
    for k, name in enumerate(HMC):
        jobs.append((f"hmc_{name}", name, "hmc", {"maxiter": 200, "nleap": 10, "stepsize": 0.01, "seed": 200 + k}, None,
                     False))
    jobs.append(("mcmc_sphere_x0", "sphere", "mcmc", {"maxiter": 1000, "stepsize": 0.05, "perc": 1.0, "seed": 31}, x0, False))
    jobs.append(("hmc_rastrigin_x0", "rastrigin", "hmc", {"maxiter": 200, "nleap": 10, "stepsize": 0.01, "seed": 32}, x0,
                 False))
    jobs.append(("mcmc_rosenbrock_cb", "rosenbrock", "mcmc", {"maxiter": 60, "stepsize": 0.05, "perc": 0.5, "seed": 41}, None,
                 True))
    jobs.append(("hmc_sphere_cb", "sphere", "hmc", {"maxiter": 40, "nleap": 10, "stepsize": 0.01, "seed": 42}, None, True))
    for tag, objective, method, options, start, with_cb in jobs:
        case, xall, funall = run(tag, objective, method, options, start, with_cb)
        cases.append(case)
        arrays[tag + "__xall"], arrays[tag + "__funall"] = xall, funall
        print(tag, "accept_ratio", float.fromhex(case["result"]["accept_ratio"]))
    with open(os.path.join(HERE, "sample.json"), "w") as f:
        json.dump({"cases": cases}, f, indent=1)
    np.savez_compressed(os.path.join(HERE, "sample_xall.npz"), **arrays)
    for name in ("sample.json", "sample_xall.npz"):
        print("wrote", name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
