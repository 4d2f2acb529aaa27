#!/usr/bin/env python3
"""How far the samplers' numpy restatement (tests/_sample_oracle.py) moves when every objective and gradient value is
changed at random by one unit in the last place: the restatement's own error, which a parity tolerance has to leave
room for.  CPU only; this is where the choice of hmc objectives in tests/test_gpu_sample.py comes from.

    python tools/sample_sensitivity.py [--chains 200] [--maxiter 30]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sample_oracle as so  # noqa: E402
from oracle import objectives  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--maxiter", type=int, default=30)
    args = ap.parse_args()
    rs = np.random.RandomState(0)

    def ulp(f):
        return np.nextafter(f, f + rs.choice([-1.0, 1.0], size=np.shape(f)))

    for name in ("sphere", "rastrigin", "ackley", "griewank", "styblinski_tang"):
        for ndim, jac in ((3, None), (8, None), (3, "analytic"), (8, "analytic"), (64, "analytic")):
            bounds = [[-5.12, 5.12]] * ndim
            opts = dict(maxiter=args.maxiter, nleap=10, stepsize=0.01, jac=jac, seed=99, rng="philox", chains=args.chains)
            fun, grad = objectives.OBJECTIVES[name], so.GRADIENTS[name]
            with np.errstate(all="ignore"):
                a = so.sample(name, bounds, method="hmc", options=dict(opts))
                objectives.OBJECTIVES[name] = lambda X: ulp(fun(X))
                so.GRADIENTS[name] = lambda X: ulp(grad(X))
                try:
                    b = so.sample(name, bounds, method="hmc", options=dict(opts))
                finally:
                    objectives.OBJECTIVES[name], so.GRADIENTS[name] = fun, grad
                print(f"{name:16s} ndim {ndim:3d} jac {str(jac):9s} max |dx| / range "
                      f"{np.abs(a.xall - b.xall).max() / 10.24:.2e}  max rel df "
                      f"{np.max(np.abs(a.funall - b.funall) / np.abs(a.funall)):.2e}  same accept counts "
                      f"{np.array_equal(a.nacc, b.nacc)}")


if __name__ == "__main__":
    main()
