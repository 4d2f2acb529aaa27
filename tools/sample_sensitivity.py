#!/usr/bin/env python3
"""How far the samplers' numpy restatement (tests/_sample_oracle.py) moves when every objective and gradient value is
changed at random by one unit in the last place: the restatement's own error, which a parity tolerance has to leave
room for.  CPU only; this is where the choice of hmc objectives in tests/test_gpu_sample.py comes from.

    python tools/sample_sensitivity.py [--chains 200] [--maxiter 30]
    python tools/sample_sensitivity.py --edges      the short hmc chains of tests/_sample_edges.py HMC_CASES, one line per
                                                    case (profiles/sample_edges_sensitivity.txt: a case's x tolerance in
                                                    tests/test_gpu_sample_edges.py is 1000 times the deviation printed here)
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


def edges(ulp):
    """Every case of tests/_sample_edges.py HMC_CASES: the restatement's run as the test runs it, and once more with every
    objective and gradient value one unit in the last place off."""
    import _sample_edges as edges_table

    print(f"restatement alone, rng=philox, seed {edges_table.HMC_SEED}, bounds [{edges_table.LOWER}, {edges_table.UPPER}], "
          f"chains {edges_table.HMC_CHAINS}, maxiter {edges_table.HMC_MAXITER}, nleap {edges_table.HMC_NLEAP}; every objective "
          "and gradient value moved at random by one unit in the last place")
    for case in edges_table.HMC_CASES:
        name, ndim, _ = case
        fun, grad = objectives.OBJECTIVES[name], so.GRADIENTS[name]
        a = edges_table.hmc_reference(case)
        objectives.OBJECTIVES[name] = lambda X: ulp(fun(X))
        so.GRADIENTS[name] = lambda X: ulp(grad(X))
        try:
            with np.errstate(all="ignore"):
                b = so.sample(name, edges_table.bounds(ndim), x0=edges_table.hmc_x0(name, ndim), method="hmc",
                              options=edges_table.hmc_options(case))
        finally:
            objectives.OBJECTIVES[name], so.GRADIENTS[name] = fun, grad
        with np.errstate(all="ignore"):
            df = np.max(np.abs(a.funall - b.funall) / np.abs(a.funall))
        print(f"{edges_table.hmc_id(case):32s} max |dx| / range {np.abs(a.xall - b.xall).max() / edges_table.SPAN:.2e}  "
              f"max rel df {df:.2e}  same accept counts {np.array_equal(a.nacc, b.nacc)}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=200)
    ap.add_argument("--maxiter", type=int, default=30)
    ap.add_argument("--edges", action="store_true", help="the table of tests/_sample_edges.py instead")
    args = ap.parse_args()
    rs = np.random.RandomState(0)

    def ulp(f):
        return np.nextafter(f, f + rs.choice([-1.0, 1.0], size=np.shape(f)))

    if args.edges:
        return edges(ulp)
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
