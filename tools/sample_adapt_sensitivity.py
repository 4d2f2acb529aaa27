#!/usr/bin/env python3
"""How far the adapting samplers' numpy restatement (tests/_sample_adapt_oracle.py) moves when every objective and gradient
value is changed at random by one unit in the last place: the restatement's own error on the parity cases of
tests/_sample_adapt_cases.py, which the tolerances of tests/test_gpu_sample_adapt.py have to leave room for.  CPU only.
All samples are compared (burn 0, thin 1), whatever the case records.

    python tools/sample_adapt_sensitivity.py            one line per case
    python tools/sample_adapt_sensitivity.py --loop     the same cases at the default target_accept too: the feedback loop
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sample_adapt_cases as cases  # noqa: E402
import _sample_adapt_oracle as ao  # noqa: E402
from oracle import objectives  # noqa: E402


def moved(case, rs, default_target=False):
    method, name = case[0], case[1]
    bounds, x0, o = cases.setup(case)
    o.update(burn=0, thin=1)
    if default_target:
        o.pop("target_accept", None)

    def ulp(f):
        return np.nextafter(f, f + rs.choice([-1.0, 1.0], size=np.shape(f)))

    fun, grad = objectives.OBJECTIVES[name], ao.GRADIENTS[name]
    a = ao.sample(name, bounds, x0=x0, method=method, options=dict(o))
    objectives.OBJECTIVES[name] = lambda X: ulp(fun(X))
    ao.GRADIENTS[name] = lambda X: ulp(grad(X))
    try:
        b = ao.sample(name, bounds, x0=x0, method=method, options=dict(o))
    finally:
        objectives.OBJECTIVES[name], ao.GRADIENTS[name] = fun, grad
    with np.errstate(all="ignore"):
        return (np.abs(a.xall - b.xall).max() / 10.24, np.nanmax(np.abs(a.funall - b.funall) / np.abs(a.funall)),
                np.max(np.abs(a.stepsizes / b.stepsizes - 1.0)), np.array_equal(a.nacc, b.nacc), o.get("target_accept"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", action="store_true", help="also every case at its default target_accept")
    args = ap.parse_args()
    rs = np.random.RandomState(0)
    print(f"restatement alone, maxiter {cases.MAXITER}, warmup {cases.WARMUP}; every objective and gradient value moved at "
          "random by one unit in the last place")
    for case in cases.PARITY:
        for default in ((False, True) if args.loop and "target_accept" in case[4] else (False,)):
            dx, df, ds, same, target = moved(case, rs, default)
            print(f"{cases.case_id(case):58s} target {str(target):5s} max |dx| / range {dx:.1e}  max rel df {df:.1e}  "
                  f"max rel dstep {ds:.1e}  same accept counts {same}", flush=True)


if __name__ == "__main__":
    main()
