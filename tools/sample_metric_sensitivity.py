#!/usr/bin/env python3
"""What the tests of metric="diag" take from the numpy restatement alone (tests/_sample_metric_oracle.py).  CPU only.

    python tools/sample_metric_sensitivity.py            one line per parity case of tests/_sample_metric_cases.py: how far
                                                         the restatement moves when every objective and gradient value is
                                                         changed at random by one unit in the last place (all samples are
                                                         compared: burn 0, thin 1).  A case is admitted under 1e-8 of the
                                                         range in xall and 1e-8 relative in stepsizes and metric.  -> profiles/sample_metric_sensitivity.txt
    python tools/sample_metric_sensitivity.py --gauss    the anisotropic Gaussian, five seeds: the smallest per-axis normalised
                                                         squared jump distance after the warm-up with the per-axis scales and
                                                         with the scalar warm-up, their ratio, and the learnt ratio of scales
                                                         -> profiles/sample_metric_cases.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _sample_metric_cases as cases  # noqa: E402
import _sample_metric_oracle as mo  # noqa: E402
from oracle import objectives  # noqa: E402

LIMIT = 1.0e-8


def moved(case, rs, **lengths):
    method, name = case[0], case[1]
    bounds, x0, o = cases.setup(case, **lengths)
    o.update(burn=0, thin=1)

    def ulp(f):
        return np.nextafter(f, f + rs.choice([-1.0, 1.0], size=np.shape(f)))

    fun, grad = objectives.OBJECTIVES[name], mo.GRADIENTS[name]
    a = mo.sample(name, bounds, x0=x0, method=method, options=dict(o))
    objectives.OBJECTIVES[name] = lambda X: ulp(fun(X))
    mo.GRADIENTS[name] = lambda X: ulp(grad(X))
    try:
        b = mo.sample(name, bounds, x0=x0, method=method, options=dict(o))
    finally:
        objectives.OBJECTIVES[name], mo.GRADIENTS[name] = fun, grad
    with np.errstate(all="ignore"):
        return (np.abs(a.xall - b.xall).max() / 10.24,
                np.max(np.abs(a.stepsizes / b.stepsizes - 1.0)), np.max(np.abs(a.metric / b.metric - 1.0)),
                np.array_equal(a.nacc, b.nacc), float(np.min(a.metric)), float(np.max(a.metric)))


def gauss():
    print("anisotropic Gaussian, sigma = geomspace(0.02, 1, 8), bounds +-5, 64 chains from x0 = 0; the restatement alone\n"
          "slowest = min over axes of E[(x_{t+1} - x_t)^2] / sigma_e^2 over the samples after the warm-up")
    for method in ("mcmc", "hmc"):
        ratios = []
        for seed in cases.GAUSS_SEEDS:
            got = {}
            for metric in (None, "diag"):
                o = cases.gauss_options(method, seed, metric)
                r = mo.sample(cases.gauss_value, cases.GAUSS_BOUNDS, x0=np.zeros(8), method=method,
                              options=dict(o, jac=cases.gauss_gradient) if method == "hmc" else o)
                got[metric] = (cases.slowest_jump(r.xall), r)
            scales = got["diag"][1].metric
            ratios.append(got["diag"][0] / got[None][0])
            print(f"{method:4s} {cases.GAUSS[method]} seed {seed}: slowest scalar {got[None][0]:.6g}  with the scales "
                  f"{got['diag'][0]:.6g}  ratio {ratios[-1]:.4g}  metric[:, -1] / metric[:, 0] mean {np.mean(scales[:, -1] / scales[:, 0]):.4g}"
                  f"  pooled variance of the widest axis {got[None][1].xall[..., -1].var():.3f} -> {got['diag'][1].xall[..., -1].var():.3f}",
                  flush=True)
        print(f"{method:4s} smallest ratio {min(ratios):.4g}: the tests' bound is half of it, {0.5 * min(ratios):.4g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gauss", action="store_true", help="the statistical figures instead of the sensitivity table")
    args = ap.parse_args()
    if args.gauss:
        return gauss()
    rs = np.random.RandomState(0)
    print(f"restatement alone, maxiter {cases.MAXITER}, warmup {cases.WARMUP} (ndim 2048: {cases.WIDE_MAXITER}, {cases.WIDE_WARMUP}), metric diag; every objective and gradient value "
          f"moved at random by one unit in the last place; admitted under {LIMIT:g} (xall: of the range 10.24; stepsizes, metric: relative)")
    wide = {"maxiter": cases.WIDE_MAXITER, "warmup": cases.WIDE_WARMUP}
    for case, lengths in [(case, {}) for case in cases.PARITY] + [(case, wide) for case in cases.WIDE]:
        dx, ds, dm, same, mlo, mhi = moved(case, rs, **lengths)
        verdict = "ok" if max(dx, ds, dm) < LIMIT else "TOO SENSITIVE"
        print(f"{cases.case_id(case):58s} max |dx| / range {dx:.1e}  max rel dstep {ds:.1e}  "
              f"max rel dmetric {dm:.1e}  same accept counts {same}  metric {mlo:.3f} ... {mhi:.3f}  {verdict}", flush=True)


if __name__ == "__main__":
    main()
