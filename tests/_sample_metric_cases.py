"""What tests/test_gpu_sample_metric.py, tests/test_sample_metric_host.py and tools/sample_metric_sensitivity.py share: the
parity cases of metric="diag" and the anisotropic Gaussian on which the per-axis scales are shown to adapt.

The parity cases run maxiter 60, warmup 40: windows (6, 16] and (16, 36].  As in tests/_sample_adapt_cases.py a case is
admitted only where the rule, a feedback loop, is well conditioned: the restatement run twice, once with every objective and
gradient value one unit in the last place off, moves by less than 1e-8 relative in xall, stepsizes and metric
(tools/sample_metric_sensitivity.py prints the table, kept in profiles/sample_metric_sensitivity.txt), so the test's 1e-6
leaves two orders for the kernels' own rounding.  That is why hmc runs on sphere with a high target_accept.
"""
import numpy as np

MAXITER, WARMUP = 60, 40
A = {"jac": "analytic"}

# (method, objective, ndim, chains, options, constraints, x0 form, (burn, thin) or None for the default burn = warmup)
# ndim: either side of the row-width thresholds (16 lanes up to 64, 32 up to 128, 64 beyond); chains 1 / 5 / 37: a last
# workgroup that is partly idle; perc 0.3: blocks that do not divide ndim; perc 0.0: one variable per sample
PARITY = [
    ("mcmc", "sphere", 3, 1, {"stepsize": 0.05, "perc": 1.0}, None, None, (7, 3)),
    ("mcmc", "rosenbrock", 64, 5, {"stepsize": 0.05, "perc": 0.3}, "Reject", "shared", None),
    ("mcmc", "rastrigin", 65, 37, {"stepsize": 0.02, "perc": 1.0, "target_accept": 0.5}, None, "per-chain", None),
    ("mcmc", "sphere", 128, 5, {"stepsize": 0.05, "perc": 0.0}, "Reject", None, None),        # k = 1: target 0.44
    ("mcmc", "rosenbrock", 129, 37, {"stepsize": 0.001, "perc": 0.3}, None, "shared", None),
    ("mcmc", "rastrigin", 300, 5, {"stepsize": 0.5, "perc": 1.0}, None, None, None),
    ("hmc", "sphere", 3, 1, dict(A, stepsize=0.01, nleap=4, target_accept=0.95), None, None, None),   # (nleap 10: 1.2e-8)
    ("hmc", "sphere", 64, 37, dict(A, stepsize=0.05, nleap=5, target_accept=0.95), "Reject", "per-chain", (7, 3)),
    ("hmc", "sphere", 65, 5, dict(A, stepsize=0.0005, nleap=5, target_accept=0.95), None, "shared", None),
    ("hmc", "sphere", 128, 37, dict(A, stepsize=0.01, nleap=3, target_accept=0.95), None, None, None),
    ("hmc", "sphere", 129, 5, dict(A, stepsize=0.2, nleap=3, target_accept=0.95), "Reject", None, None),
    ("hmc", "sphere", 300, 37, dict(A, stepsize=0.01, nleap=3, target_accept=0.95), None, "per-chain", None),
    ("hmc", "sphere", 3, 5, {"stepsize": 0.01, "nleap": 4, "jac": None, "target_accept": 0.99}, None, "per-chain", None),
    ("hmc", "sphere", 8, 37, {"stepsize": 0.05, "nleap": 3, "jac": None, "target_accept": 0.98}, "Reject", None, None),
]


# the LDS limit of the row with eff: ndim 2048, 2 chains, maxiter 24, warmup 20 (one window, (3, 18]); mcmc and analytic hmc
WIDE_MAXITER, WIDE_WARMUP = 24, 20
WIDE = [
    ("mcmc", "sphere", 2048, 2, {"stepsize": 0.002, "perc": 1.0}, None, None, None),
    ("hmc", "sphere", 2048, 2, dict(A, stepsize=0.002, nleap=3, target_accept=0.95), None, None, None),
]


def case_id(case):
    method, objective, ndim, chains, options, constraints, x0, rec = case
    return f"{method}-{objective}-{ndim}-{chains}-{options.get('jac', '')}-{constraints}-{x0}-{rec}"


def setup(case, maxiter=MAXITER, warmup=WARMUP):
    """(bounds, x0, options) of a case, as the test and the tool run it."""
    method, objective, ndim, chains, options, constraints, x0, rec = case
    bounds = [[-5.12, 5.12]] * ndim
    rs = np.random.RandomState(ndim + chains)
    start = {None: None, "shared": rs.uniform(-2, 2, ndim), "per-chain": rs.uniform(-2, 2, (chains, ndim))}[x0]
    if x0 == "per-chain" and chains == 1:
        start = start[0]
    o = dict(options, maxiter=maxiter, warmup=warmup, metric="diag", seed=31 + ndim, chains=chains, constraints=constraints,
             rng="philox")
    if rec is not None:
        o["burn"], o["thin"] = rec
    return bounds, start, o


# ---- the anisotropic Gaussian: -log p = 0.5 sum (x / sigma)^2, sigma = geomspace(0.02, 1, 8), bounds +-5, 64 chains from 0 ----
SIGMA = np.geomspace(0.02, 1.0, 8)
GAUSS_BOUNDS = [[-5.0, 5.0]] * 8
GAUSS_CHAINS = 64
GAUSS_SEEDS = (0, 1, 2, 3, 4)
GAUSS = {"mcmc": {"maxiter": 2000, "warmup": 1500, "perc": 1.0},
         "hmc": {"maxiter": 800, "warmup": 600, "nleap": 10, "stepsize": 0.01}}
# Bounds on (smallest normalised squared jump distance with the scales) / (the same with the scalar warm-up alone): HALF the
# smallest of the five ratios the restatement gives on the CPU, profiles/sample_metric_cases.txt (mcmc 146.3, hmc 11.33)
GAUSS_RATIO_BOUND = {"mcmc": 0.5 * 146.3, "hmc": 0.5 * 11.33}
SCALE_RATIO_EXACT = 50.0  # sigma[-1] / sigma[0]; the learnt metric[:, -1] / metric[:, 0] (mean over chains) within a factor 2


def gauss_value(X):
    return 0.5 * ((X / SIGMA) ** 2).sum(axis=-1)


def gauss_gradient(X):
    return X / SIGMA ** 2


def gauss_options(method, seed, metric):
    return dict(GAUSS[method], chains=GAUSS_CHAINS, seed=seed, rng="philox", metric=metric, burn=GAUSS[method]["warmup"] + 1)


def slowest_jump(xall):
    """xall (C, rows, n), consecutive samples after the warm-up: the squared jump distance per sample E[(x_{t+1} - x_t)^2] /
    sigma_e^2, over chains and samples, on the axis where it is smallest."""
    d = np.diff(np.asarray(xall), axis=1)
    return float(((d * d).mean(axis=(0, 1)) / SIGMA ** 2).min())
