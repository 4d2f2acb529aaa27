#!/usr/bin/env python3
"""What the tests of the moves of method="ensemble" take from the numpy restatement alone (tests/_ensemble_moves_oracle.py).
CPU only.

    python tools/sample_ensemble_moves_cases.py [--jobs N]
        the rotated Gaussian and the bimodal mixture of tests/_ensemble_moves_cases.py, seeds 0 ... 4: per run the smallest and
        the largest per-axis variance over sigma^2 (the share of the samples in the heavy mode) of the samples kept, the
        acceptance ratio, and the largest deviation per run (the tests bound theirs by three times it); the stretch move alone
        on the bimodal target.  -> profiles/sample_ensemble_moves_cases.txt
"""
import argparse
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ensemble_moves_cases as cases  # noqa: E402
import _ensemble_moves_oracle  # noqa: E402


def gauss(job):
    name, seed = job
    x0, o = cases.gauss_options(name, seed)
    res = _ensemble_moves_oracle.sample(cases.rotated_value, cases.GAUSS_BOUNDS, x0=x0, options=o)
    r = cases.variance_ratio(res.xall, cases.GAUSS_RUNS[name][2])
    return name, seed, float(r.min()), float(r.max()), res.accept_ratio


def bimodal(job):
    name, seed = job
    moves = cases.BIMODAL_MOVES.get(name)  # (None: the stretch move alone)
    res = _ensemble_moves_oracle.sample(cases.bimodal_value, cases.BIMODAL_BOUNDS, options=cases.bimodal_options(moves, seed))
    share, each = cases.heavy_share(res.xall)
    return name, seed, share, float(each.min()), float(each.max()), res.accept_ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    gauss_jobs = [(name, seed) for name in cases.GAUSS_RUNS for seed in cases.SEEDS]
    bimodal_jobs = [(name, seed) for name in list(cases.BIMODAL_MOVES) + ["stretch"] for seed in cases.SEEDS]
    with ProcessPoolExecutor(args.jobs) as pool:
        gauss_rows = list(pool.map(gauss, gauss_jobs))
        bimodal_rows = list(pool.map(bimodal, bimodal_jobs))
    lines = [f"method=\"ensemble\" with moves, restatement on the CPU: {cases.ENSEMBLES} ensembles of {cases.WALKERS} walkers.",
             "Rotated Gaussian: per-axis variance / sigma^2 in the rotated frame of the samples kept (de, snooker: x0 from the target, "
             "3000 samples, from 1000 on; mixture = " + repr(cases.MIXTURE) + ": x0=None, 1500 samples, from 750 on)",
             "run       seed  min     max     accept_ratio"]
    worst = {}
    for name, seed, lo, hi, acc in gauss_rows:
        worst[name] = max(worst.get(name, 0.0), abs(lo - 1.0), abs(hi - 1.0))
        lines.append(f"{name:9s} {seed:4d}  {lo:.4f}  {hi:.4f}  {acc:.4f}")
    for name, dev in worst.items():
        lines.append(f"{name}: largest |variance / sigma^2 - 1| {dev:.4f}   bound of the tests (three times it): {3.0 * dev:.4f}")
    lines += ["Bimodal target 0.75 N(+2 e0, 0.25^2 I) + 0.25 N(-2 e0, 0.25^2 I), 4 dimensions, x0=None, 2000 samples, second half kept: "
              "the share of the samples with x0 > 0 (exact: 0.75), pooled and the smallest / largest of an ensemble",
              "run         seed  share   min     max     accept_ratio"]
    worst = {}
    for name, seed, share, lo, hi, acc in bimodal_rows:
        worst[name] = max(worst.get(name, 0.0), abs(share - cases.BIMODAL_SHARE))
        lines.append(f"{name:11s} {seed:4d}  {share:.4f}  {lo:.4f}  {hi:.4f}  {acc:.4f}")
    for name, dev in worst.items():
        if name == "stretch":
            least = min(abs(r[2] - cases.BIMODAL_SHARE) for r in bimodal_rows if r[0] == "stretch")
            lines.append(f"stretch: misses 0.75 by {least:.4f} to {dev:.4f} (the tests require more than {cases.STRETCH_MISSES_BY})")
        else:
            lines.append(f"{name}: largest |share - 0.75| {dev:.4f}   bound of the tests (three times it): {3.0 * dev:.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "sample_ensemble_moves_cases.txt"), "w") as out:
        out.write(text)


if __name__ == "__main__":
    main()
