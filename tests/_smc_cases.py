"""What tests/test_sample_smc_host.py, tests/test_gpu_sample_smc.py and tools/sample_smc_cases.py share: the targets on which
method="smc" is shown to sample correctly and to return the evidence, the statistics and their bounds, the parity cases and
how their seeds are admitted, and the objectives that plant values.

Sphere in 4 dimensions, box +-5.12 (oracle.objectives' sphere: the posterior is N(0, I / 2)): 16 populations of 1 024 particles,
8 steps.  Statistics: the pooled log-evidence ``logaddexp.reduce(log_evidence) - log C`` against
``4 log(sqrt(pi) erf(5.12) / 10.24)``, and the pooled variance per axis against 0.5.

Bimodal target of tests/_ensemble_moves_cases.py (0.75 N(+2 e0, 0.25^2 I) + 0.25 N(-2 e0, 0.25^2 I), 4 dimensions, box +-5):
32 populations of 1 024 particles, 8 steps.  Statistics: the pooled log-evidence against ``2 log(2 pi 0.0625) - 4 log 10`` and
the share of the particles with x0 > 0 against 0.75.  (With 16 populations the largest deviation of the log-evidence over the
five seeds was 0.0765, three times which is above the cap of 0.2 the bound must stay under: the run was enlarged, not the cap.)
"""
import math

import numpy as np

from _ensemble_moves_cases import BIMODAL_BOUNDS, BIMODAL_SHARE, bimodal_value  # noqa: F401

SEEDS = (0, 1, 2, 3, 4)
TEST_SEEDS = (1, 3)  # the two the host tests run
GPU_SEED = 1         # the one the GPU tests run

SPHERE_BOUNDS = [[-5.12, 5.12]] * 4
SPHERE_OPTIONS = {"chains": 16, "particles": 1024, "steps": 8, "ess": 0.5}
SPHERE_LOGZ = 4.0 * math.log(math.sqrt(math.pi) * math.erf(5.12) / 10.24)
SPHERE_VARIANCE = 0.5
BIMODAL_OPTIONS = {"chains": 32, "particles": 1024, "steps": 8, "ess": 0.5}
BIMODAL_LOGZ = 2.0 * math.log(2.0 * math.pi * 0.0625) - 4.0 * math.log(10.0)

# The largest deviation of each statistic over the five seeds, from the restatement on the CPU (profiles/sample_smc_cases.txt,
# written by tools/sample_smc_cases.py) with the seed that produced it, and the tests' bounds: three times that -- the margin
# covers the sampling noise over five seeds, as in tests/_ensemble_moves_cases.py.
LARGEST_DEVIATION = {
    "sphere_logz": 0.0193,      # seed 3
    "sphere_variance": 0.0135,  # seed 4
    "bimodal_logz": 0.0216,     # seed 4
    "bimodal_share": 0.0066,    # seed 1
}
BOUND = {k: 3.0 * v for k, v in LARGEST_DEVIATION.items()}
CAP = {"sphere_logz": 0.2, "bimodal_logz": 0.2, "sphere_variance": 0.05, "bimodal_share": 0.05}  # what a bound may not exceed
MCMC_MISSES_BY = 0.15  # the target discriminates: plain mcmc chains from a uniform start miss the share 0.75 by more than this


def pooled_log_evidence(log_evidence):
    log_evidence = np.atleast_1d(log_evidence)
    return float(np.logaddexp.reduce(log_evidence) - math.log(len(log_evidence)))


def sphere_statistics(res):
    """(|pooled log-evidence - exact|, the largest |pooled variance per axis - 0.5|)."""
    var = np.asarray(res.xall).reshape(-1, 4).var(axis=0)
    return abs(pooled_log_evidence(res.log_evidence) - SPHERE_LOGZ), float(np.max(np.abs(var - SPHERE_VARIANCE)))


def bimodal_statistics(res):
    """(|pooled log-evidence - exact|, |share of the heavy mode - 0.75|)."""
    share = float((np.asarray(res.xall)[..., 0] > 0.0).mean())
    return abs(pooled_log_evidence(res.log_evidence) - BIMODAL_LOGZ), abs(share - BIMODAL_SHARE)


# ---- parity with the restatement ------------------------------------------------------------------------------------------
# (objective, ndim, particles, populations, maxiter): every factory objective; ndim on both sides of the boundaries of the three
# lanes-per-row forms (64 | 65, 128 | 129) and one row past 256; P below, at and off one wave of row groups and past one pass of
# the stage kernel's 1 024 threads.  The long rows stop after a few stages (status -1): their ladders have hundreds.
PARITY = [
    ("sphere", 1, 4, 1, 100),
    ("sphere", 2, 63, 3, 100),
    ("ackley", 3, 64, 1, 100),
    ("griewank", 64, 100, 1, 3),
    ("quartic", 65, 64, 3, 3),
    ("rastrigin", 128, 63, 1, 3),
    ("rosenbrock", 129, 100, 1, 3),
    ("styblinski_tang", 300, 64, 1, 3),
    ("sphere", 3, 1025, 3, 100),
    ("rosenbrock", 2, 1025, 1, 100),
    ("ackley", 64, 4, 3, 3),
    ("griewank", 2, 100, 3, 100),
    ("quartic", 3, 1025, 1, 100),
    ("rastrigin", 65, 4, 1, 3),
    ("styblinski_tang", 128, 100, 3, 3),
    ("sphere", 300, 4, 3, 2),
    ("rosenbrock", 300, 63, 1, 2),
    ("sphere", 129, 64, 1, 3),
    ("ackley", 1, 1025, 1, 100),
    ("griewank", 300, 100, 1, 2),
]
PARITY_STEPS = 3
PARITY_BOUND = 5.12


def parity_id(case):
    return "%s-n%d-P%d-C%d" % case[:4]


def parity_setup(case):
    """(objective's name, bounds, options) of a parity case; the seed is where the admission starts."""
    fun, n, P, C, maxiter = case
    return fun, [[-PARITY_BOUND, PARITY_BOUND]] * n, {"chains": C, "particles": P, "steps": PARITY_STEPS, "maxiter": maxiter,
                                                     "seed": 10 * PARITY.index(case)}


def moved_by_at_most(a, b, tol):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(a)))))


_admitted = {}


def admitted(case, tries=8):
    """(seed, the restated run with its per-stage records): a parity tolerance only means something where the restatement's own
    rounding stays well inside it -- the first seed from the case's own on whose restated run keeps every ancestor and every
    acceptance count, and moves betas / log_evidence by at most 1e-9, when each objective value, each weight and each running sum
    is moved at random by one unit in the last place (the method of tests/_ensemble_moves_cases.admitted).  The restatement alone
    decides.  Computed once per case and left unchanged."""
    if case in _admitted:
        return _admitted[case]
    import _smc_oracle
    from oracle import objectives

    fun, bounds, opts = parity_setup(case)
    f = objectives.OBJECTIVES[fun]
    rs = np.random.RandomState(0)

    def nudge(v):
        v = np.asarray(v, dtype=np.float64)
        return np.nextafter(v, v + rs.choice([-1.0, 1.0], size=v.shape))

    def moved(X):
        return nudge(f(X))

    for seed in range(opts["seed"], opts["seed"] + tries):
        o = dict(opts, seed=seed)
        a = _smc_oracle.sample(f, bounds, dict(o), record=True)
        b = _smc_oracle.sample(moved, bounds, dict(o), nudge=nudge, record=True)
        same = a.nit == b.nit and np.array_equal(a.statuses, b.statuses) and \
            all(np.array_equal(p, q) for p, q in zip(a.ancs, b.ancs)) and all(np.array_equal(p, q) for p, q in zip(a.naccs, b.naccs))
        if same and moved_by_at_most(a.betas, b.betas, 1e-9) and moved_by_at_most(a.log_evidence, b.log_evidence, 1e-9):
            _admitted[case] = (seed, a)
            return _admitted[case]
    raise AssertionError("no admissible seed")


# ---- objectives that plant values ---------------------------------------------------------------------------------------------
# An objective that ignores where its rows are and returns one fixed value per row: the same rule for the restatement (numpy) and,
# tagged with factory.batched, for the device (a tensor).
PLANT_P, PLANT_NDIM = 64, 3
PLANT_BOUNDS = [[-1.0, 2.0]] * PLANT_NDIM


def plant_constant(C=1):
    return np.full(C * PLANT_P, 2.5)


def plant_one_finite(which=37):
    v = np.where(np.arange(PLANT_P) % 2 == 0, np.inf, np.nan)
    v[which] = 1.0
    return v


def plant_mixed(middle):
    """Three populations: the outer two hold fixed finite values, the middle one what ``middle`` says: "none" (no finite
    value) or "neginf" (finite values and one -inf)."""
    rs = np.random.RandomState(7)
    v = rs.uniform(0.0, 6.0, size=3 * PLANT_P)
    if middle == "none":
        v[PLANT_P:2 * PLANT_P] = np.where(np.arange(PLANT_P) % 3 == 0, np.nan, np.inf)
    else:
        v[PLANT_P + 11] = -np.inf
    return v


def planted(values):
    """The restatement's objective."""
    values = np.asarray(values, dtype=np.float64)

    def fun(X):
        assert len(X) == len(values)
        return values.copy()

    return fun
