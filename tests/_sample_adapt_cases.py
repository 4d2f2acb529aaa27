"""The parity cases of tests/test_gpu_sample_adapt.py, shared with tools/sample_adapt_sensitivity.py (which measures, on the
CPU and from the restatement alone, how far each case moves under its OWN rounding).

Why the cases set ``target_accept`` for hmc.  The rule is a feedback loop: the multiplier sets the trajectory, the trajectory
sets alpha, alpha sets the next multiplier, with a gain of sqrt(t) / (0.05 (t + 10)) (up to 3.2, at t = 10) times
d alpha / d log s.  Where alpha depends strongly on the step -- hmc at its default target 0.65 on rows of 64 elements, or any
hmc with finite differences, whose gradient carries a rounding error of 1e-16 f / h -- a difference in the last place grows by
a factor of about three per warm-up sample, and after 40 of them two correct implementations share no digit: the restatement
run twice, once with every objective and gradient value one unit in the last place off, differs by 0.36 of the search range
on (hmc, sphere, 64, 37 chains, stepsize 0.05, nleap 5, default target).  A comparison at 1e-6 there would test the rounding,
not the kernel (tests/test_gpu_sample.py chooses its hmc objectives for the same reason).  Near a high target alpha is flat
in the step and the loop is stable.  Every case below moves by less than 1e-9 of the range, 1e-9 relative in the multipliers
and 4e-8 relative in funall under that experiment (tools/sample_adapt_sensitivity.py prints the table, kept in
profiles/sample_adapt_sensitivity.txt; most cases stay under 1e-10), so the tolerances of the test (1e-6) leave a factor of 25
and mostly three orders for the kernels' own rounding.  The default targets are covered by
the mcmc cases, by the one-chain hmc case, and statistically by test_it_adapts.
"""
import numpy as np

MAXITER, WARMUP = 60, 40
A = {"jac": "analytic"}

# (method, objective, ndim, chains, options, constraints, x0 form, (burn, thin) or None for the default burn = warmup)
# ndim: either side of the row-width thresholds (16 lanes up to 64, 32 up to 128, 64 beyond); chains 1 / 5 / 37: a last
# workgroup that is partly inactive; perc 0.3 / 0.5: blocks that do not divide ndim; perc 0.0: one variable per sample
PARITY = [
    ("mcmc", "sphere", 3, 1, {"stepsize": 0.05, "perc": 1.0}, None, None, (7, 3)),
    ("mcmc", "rosenbrock", 64, 5, {"stepsize": 0.05, "perc": 0.3}, "Reject", "shared", None),
    ("mcmc", "rastrigin", 65, 37, {"stepsize": 0.02, "perc": 0.5, "target_accept": 0.5}, None, "per-chain", (7, 3)),
    ("mcmc", "sphere", 128, 5, {"stepsize": 0.05, "perc": 0.0}, "Reject", None, None),        # k = 1: target 0.44
    ("mcmc", "rosenbrock", 129, 37, {"stepsize": 0.001, "perc": 0.3}, None, "shared", (7, 3)),
    ("mcmc", "rastrigin", 300, 5, {"stepsize": 0.5, "perc": 1.0}, None, None, None),
    ("hmc", "sphere", 3, 1, dict(A, stepsize=0.01, nleap=10), None, None, None),               # the default target, 0.65
    ("hmc", "sphere", 64, 37, dict(A, stepsize=0.05, nleap=5, target_accept=0.95), "Reject", "per-chain", (7, 3)),
    ("hmc", "sphere", 65, 5, dict(A, stepsize=0.0005, nleap=5, target_accept=0.95), None, "shared", None),
    ("hmc", "sphere", 128, 37, dict(A, stepsize=0.01, nleap=3, target_accept=0.95), None, None, (7, 3)),
    ("hmc", "sphere", 129, 5, dict(A, stepsize=0.2, nleap=3, target_accept=0.95), "Reject", None, None),
    ("hmc", "sphere", 300, 37, dict(A, stepsize=0.01, nleap=3, target_accept=0.95), None, "per-chain", (7, 3)),
    ("hmc", "sphere", 3, 5, {"stepsize": 0.01, "nleap": 4, "jac": None, "target_accept": 0.99}, None, "per-chain", (7, 3)),
    ("hmc", "sphere", 8, 37, {"stepsize": 0.05, "nleap": 3, "jac": None, "target_accept": 0.98}, "Reject", None, None),
]


def case_id(case):
    method, objective, ndim, chains, options, constraints, x0, rec = case
    return f"{method}-{objective}-{ndim}-{chains}-{options.get('jac', '')}-{constraints}-{x0}-{rec}"


def setup(case):
    """(bounds, x0, options) of a case, as the test and the tool run it."""
    method, objective, ndim, chains, options, constraints, x0, rec = case
    bounds = [[-5.12, 5.12]] * ndim
    rs = np.random.RandomState(ndim + chains)
    start = {None: None, "shared": rs.uniform(-2, 2, ndim), "per-chain": rs.uniform(-2, 2, (chains, ndim))}[x0]
    if x0 == "per-chain" and chains == 1:
        start = start[0]
    o = dict(options, maxiter=MAXITER, warmup=WARMUP, seed=31 + ndim, chains=chains, constraints=constraints, rng="philox")
    if rec is not None:
        o["burn"], o["thin"] = rec
    return bounds, start, o
