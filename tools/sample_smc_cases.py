#!/usr/bin/env python3
"""What the tests of method="smc" take from the numpy restatement alone (tests/_smc_oracle.py).  CPU only.

    python tools/sample_smc_cases.py [--jobs N]
        the sphere and the bimodal mixture of tests/_smc_cases.py, seeds 0 ... 4: per run the stages, the deviation of the pooled
        log-evidence from the exact value, the pooled variance per axis (the share of the particles in the heavy mode), the
        overall acceptance ratio, and the largest deviation per statistic with its seed (the tests bound theirs by three times
        it, which must stay under the statistic's cap); the restated mcmc chains on the bimodal target.
        -> profiles/sample_smc_cases.txt
"""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sample_oracle  # noqa: E402
import _smc_cases as cases  # noqa: E402
import _smc_oracle  # noqa: E402
from oracle import objectives  # noqa: E402


def sphere(seed):
    res = _smc_oracle.sample("sphere", cases.SPHERE_BOUNDS, dict(cases.SPHERE_OPTIONS, seed=seed))
    var = res.xall.reshape(-1, 4).var(axis=0)
    return seed, res.nit, cases.pooled_log_evidence(res.log_evidence) - cases.SPHERE_LOGZ, float(var.min()), float(var.max()), \
        res.accept_ratio


def bimodal(seed):
    res = _smc_oracle.sample(cases.bimodal_value, cases.BIMODAL_BOUNDS, dict(cases.BIMODAL_OPTIONS, seed=seed))
    each = (res.xall[..., 0] > 0.0).mean(axis=1)
    return seed, res.nit, cases.pooled_log_evidence(res.log_evidence) - cases.BIMODAL_LOGZ, float(each.mean()), float(each.min()), \
        float(each.max()), res.accept_ratio


def chains(seed):
    objectives.OBJECTIVES["bimodal"] = cases.bimodal_value
    res = _sample_oracle.sample("bimodal", cases.BIMODAL_BOUNDS, method="mcmc",
                                options={"chains": 16 * 1024, "maxiter": 57, "seed": seed, "rng": "philox", "stepsize": 0.1})
    return seed, float((res.xall[:, -1, 0] > 0.0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    with ProcessPoolExecutor(args.jobs) as pool:
        sphere_rows = list(pool.map(sphere, cases.SEEDS))
        bimodal_rows = list(pool.map(bimodal, cases.SEEDS))
        chain_rows = list(pool.map(chains, cases.SEEDS))
    worst = {}

    def note(name, seed, dev):
        if dev > worst.get(name, (-1.0, 0))[0]:
            worst[name] = (dev, seed)

    o = cases.SPHERE_OPTIONS
    lines = ['method="smc", restatement on the CPU.',
             f"Sphere in 4 dimensions, box +-5.12: {o['chains']} populations of {o['particles']} particles, {o['steps']} steps, "
             f"ess {o['ess']}.  Exact log-evidence {cases.SPHERE_LOGZ:.4f}, exact variance per axis 0.5",
             "seed  stages  dlogZ     var min  var max  accept_ratio"]
    for seed, nit, dz, lo, hi, acc in sphere_rows:
        note("sphere_logz", seed, abs(dz))
        note("sphere_variance", seed, max(abs(lo - 0.5), abs(hi - 0.5)))
        lines.append(f"{seed:4d}  {nit:6d}  {dz:+.4f}   {lo:.4f}   {hi:.4f}   {acc:.4f}")
    o = cases.BIMODAL_OPTIONS
    lines += [f"Bimodal target 0.75 N(+2 e0, 0.25^2 I) + 0.25 N(-2 e0, 0.25^2 I), 4 dimensions, box +-5: {o['chains']} populations of "
              f"{o['particles']} particles, {o['steps']} steps, ess {o['ess']}.  Exact log-evidence {cases.BIMODAL_LOGZ:.4f}; the share "
              "of the particles with x0 > 0 (exact: 0.75), pooled and the smallest / largest of a population",
              "seed  stages  dlogZ     share   min     max     accept_ratio"]
    for seed, nit, dz, share, lo, hi, acc in bimodal_rows:
        note("bimodal_logz", seed, abs(dz))
        note("bimodal_share", seed, abs(share - cases.BIMODAL_SHARE))
        lines.append(f"{seed:4d}  {nit:6d}  {dz:+.4f}   {share:.4f}  {lo:.4f}  {hi:.4f}  {acc:.4f}")
    lines.append("statistic        largest deviation (seed)   bound of the tests (three times it)   cap")
    for name in ("sphere_logz", "sphere_variance", "bimodal_logz", "bimodal_share"):
        dev, seed = worst[name]
        lines.append(f"{name:16s} largest deviation {dev:.4f} (seed {seed})   bound {3.0 * dev:.4f}   cap {cases.CAP[name]}")
    misses = [abs(share - cases.BIMODAL_SHARE) for _, share in chain_rows]
    lines.append(f"mcmc, 16 x 1024 chains from a uniform start, 57 samples, stepsize 0.1, the share of the last samples: misses 0.75 "
                 f"by {min(misses):.4f} to {max(misses):.4f} (the tests require more than {cases.MCMC_MISSES_BY})")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "sample_smc_cases.txt"), "w") as out:
        out.write(text)


if __name__ == "__main__":
    main()
