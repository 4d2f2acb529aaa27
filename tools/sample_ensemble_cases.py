#!/usr/bin/env python3
"""What the tests of method="ensemble" take from the numpy restatement alone (tests/_ensemble_oracle.py).  CPU only.

    python tools/sample_ensemble_cases.py    the anisotropic Gaussian of tests/_ensemble_cases.py, axis-aligned and rotated, seeds
                                             0 ... 4: the smallest and the largest per-axis variance over sigma^2 of the second
                                             half of the samples and the acceptance ratio; the largest deviation from 1 (the tests
                                             bound theirs by three times it); and the same statistic from the restated mcmc with
                                             its default stepsize.  -> profiles/sample_ensemble_cases.txt
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ensemble_cases as cases  # noqa: E402
import _ensemble_oracle  # noqa: E402
from _sample_metric_cases import GAUSS_BOUNDS  # noqa: E402


def main():
    lines = [f"method=\"ensemble\", restatement on the CPU: {cases.ENSEMBLES} ensembles of {cases.WALKERS} walkers, maxiter "
             f"{cases.MAXITER}, x0=None, second half kept; per-axis variance / sigma^2 (rotated target: in the rotated frame)",
             "target        seed  min     max     accept_ratio"]
    worst = 0.0
    for name, (value, frame) in cases.TARGETS.items():
        for seed in cases.SEEDS:
            res = _ensemble_oracle.sample(value, GAUSS_BOUNDS, options=cases.options(seed))
            r = cases.variance_ratio(res.xall, frame)
            worst = max(worst, float(np.abs(r - 1.0).max()))
            lines.append(f"{name:13s} {seed:4d}  {r.min():.4f}  {r.max():.4f}  {res.accept_ratio:.4f}")
            print(lines[-1], flush=True)
    lines.append(f"largest |variance / sigma^2 - 1|: {worst:.4f}   bound of the tests (three times it): {3.0 * worst:.4f}")
    seed = cases.TEST_SEEDS[0]
    r = cases.mcmc_variance_ratio(seed)
    lines.append(f"mcmc (restated, default stepsize 0.1, perc 1.0, {cases.ENSEMBLES * cases.WALKERS} chains, seed {seed}), "
                 "axis-aligned target, variance / sigma^2 per axis from the narrowest:")
    lines.append("  " + "  ".join(f"{v:.4g}" for v in r))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(os.path.join(ROOT, "profiles", "sample_ensemble_cases.txt"), "w") as out:
        out.write(text)


if __name__ == "__main__":
    main()
