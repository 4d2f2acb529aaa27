"""The case tables of tests/test_gpu_sample_edges.py (and of its host twin tests/test_sample_edges_host.py, and of
tools/sample_sensitivity.py --edges): plain data, numpy and the numpy restatement -- importable without a GPU.

The sampler kernels (csrc/sx_sample.hip, sx_sample_unfused.hip) change their path with the row length n: a row group has
LPR = 16 / 32 / 64 lanes for n <= 64 / <= 128 / larger (lanes_per_row), element e sits in lane e % LPR, elements e0 and
e0 + LPR of a lane share one Box-Muller call, and the LDS row stride changes between 256 and 257 (gen_row_stride).  The
tables put cases on both sides of each of these, and at n = 1 and 2.

Every whole run draws with rng="philox" inside [-5.12, 5.12]^n.  The reference of a run is _sample_oracle.sample, cached
here per case so that the host and the GPU test (and several GPU tests) share one evaluation.
"""
import functools
import os
import re

import numpy as np

import _sample_oracle
from oracle import objectives

ALL = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")
LOWER, UPPER = -5.12, 5.12
SPAN = UPPER - LOWER
PROJECT_XTOL = 1.0e-6  # of the range: the project's parity tolerance for samples (1e-6 relative for values)


def lanes_per_row(n):
    return 16 if n <= 64 else (32 if n <= 128 else 64)


def bounds(n):
    return [[LOWER, UPPER]] * n


# ---- A. the gradient kernel, per element ----------------------------------------------------------------------------------
GRAD_NS = (1, 2, 3, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 1030, 2048)
GRAD_ROWS = 33        # a partial last workgroup at every n (16 / 8 / 4 rows per workgroup at most)
GRAD_RTOL = 1.0e-12   # the bar of test_gpu_sample.py test_analytic_gradients, per row
GRAD_REF_RTOL = 1.0e-13  # the float64 closed form against its np.longdouble evaluation, per row


def gradient_longdouble(objective, X):
    """The closed forms of _sample_oracle.GRADIENTS carried out in np.longdouble.  The constants the kernels define their
    functions with (the double 2 pi, the double sqrt(j + 1)) stay doubles: they are part of the function, not of its rounding."""
    with np.errstate(all="ignore"):
        return _sample_oracle.GRADIENTS[objective](np.asarray(X, dtype=np.longdouble))


def _row_ok(objective, row):
    """Whether the float64 closed form of this row is good to GRAD_REF_RTOL of its norm (and, griewank: no cosine factor is
    exactly zero -- the kernel documents that it does not handle that)."""
    X = row[None, :]
    if objective == "griewank" and np.any(np.cos(X / np.sqrt(np.arange(1, X.shape[1] + 1))) == 0.0):
        return False
    with np.errstate(all="ignore"):
        want = _sample_oracle.GRADIENTS[objective](X)
    exact = gradient_longdouble(objective, X)
    if not (np.all(np.isfinite(want)) and np.all(np.isfinite(exact))):
        return False
    return float(np.linalg.norm((want - exact).astype(np.float64))) <= GRAD_REF_RTOL * float(np.linalg.norm(want))


@functools.lru_cache(maxsize=None)
def gradient_rows(objective, n):
    """(GRAD_ROWS, n) points in [-5, 5]: uniform draws, with
      row 0  all zeros (ackley's origin branch; sphere, quartic, rastrigin, griewank: a gradient of exactly 0.0),
      row 1  all ones (rosenbrock's minimum: exactly 0.0),
      row 2  zeros but 1.5 in elements LPR - 1, LPR and n - 1 (those inside the row): rosenbrock's neighbour terms across a
             lane boundary -- the last lane's right neighbour is lane 0's next trip -- and at the row's end,
      row 3  small integers (the sines of rastrigin and ackley at their zeros).
    A drawn row whose float64 reference is not good to GRAD_REF_RTOL is drawn again HERE, never skipped at run time."""
    rs = np.random.RandomState(1000 * n + ALL.index(objective))
    X = rs.uniform(-5.0, 5.0, (GRAD_ROWS, n))
    lpr = lanes_per_row(n)
    X[0] = 0.0
    X[1] = 1.0
    X[2] = 0.0
    for e in (lpr - 1, lpr, n - 1):
        if e < n:
            X[2, e] = 1.5
    X[3] = rs.randint(-4, 5, n).astype(np.float64)
    for r in range(4, GRAD_ROWS):
        for _ in range(100):
            if _row_ok(objective, X[r]):
                break
            X[r] = rs.uniform(-5.0, 5.0, n)
        else:
            raise AssertionError(f"no well-conditioned row for {objective} n = {n}")
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def gradient_reference(objective, n):
    with np.errstate(all="ignore"):
        want = _sample_oracle.GRADIENTS[objective](gradient_rows(objective, n))
    want.setflags(write=False)
    return want


# ---- B. short hmc chains against the restatement --------------------------------------------------------------------------
HMC_CHAINS, HMC_MAXITER, HMC_NLEAP, HMC_SEED = 24, 4, 2, 99
HMC_ANALYTIC_NS = (1, 2, 17, 33, 65, 128, 129, 257, 1030, 2048)
HMC_FD_NS = (2, 17, 33, 65, 130, 257)
# rosenbrock and quartic from the whole box accept nothing from n = 17 on (such a case would test rejection only): they start
# from a per-chain x0 near their valleys with a smaller step.  These are the GPU cases of x0_stride = n too.
HMC_NARROW = {"rosenbrock": (0.5, 1.5), "quartic": (-1.0, 1.0)}
HMC_CASES = tuple((name, n, jac) for jac, ns in (("analytic", HMC_ANALYTIC_NS), (None, HMC_FD_NS)) for n in ns for name in ALL)


def hmc_id(case):
    name, n, jac = case
    return f"{name}-{n}-{'analytic' if jac else 'fd'}"


def hmc_x0(name, n):
    if name not in HMC_NARROW:
        return None
    lo, hi = HMC_NARROW[name]
    return np.random.RandomState(n).uniform(lo, hi, (HMC_CHAINS, n))


def hmc_options(case):
    name, n, jac = case
    return {"maxiter": HMC_MAXITER, "nleap": HMC_NLEAP, "stepsize": 0.002 if name in HMC_NARROW else 0.01, "jac": jac,
            "seed": HMC_SEED, "rng": "philox", "chains": HMC_CHAINS, "return_all": True}


@functools.lru_cache(maxsize=None)
def hmc_reference(case):
    name, n, _ = case
    with np.errstate(all="ignore"):
        return _sample_oracle.sample(name, bounds(n), x0=hmc_x0(name, n), method="hmc", options=hmc_options(case))


SENSITIVITY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "sample_edges_sensitivity.txt")
SENSITIVITY_LINE = re.compile(r"^(\S+)\s+max \|dx\| / range (\S+)\s+max rel df (\S+)\s+same accept counts (True|False)\s*$")


@functools.lru_cache(maxsize=None)
def hmc_sensitivity():
    """{case id: (max |dx| / range, same accept counts)} as tools/sample_sensitivity.py --edges printed them: how far the
    restatement's own run moves when every objective and gradient value moves by one unit in the last place."""
    out = {}
    with open(SENSITIVITY_FILE) as f:
        for line in f:
            m = SENSITIVITY_LINE.match(line)
            if m:
                out[m.group(1)] = (float(m.group(2)), m.group(4) == "True")
    return out


def hmc_xtol(case):
    """The x tolerance of a case as a share of the range: 1000 times its printed one-ulp deviation (room for the device's
    few-ulp log / sqrt / sincos and the butterfly order of the row totals on top of a one-ulp model), at least 1e-12, and
    never more than the project's 1e-6."""
    deviation, _ = hmc_sensitivity()[hmc_id(case)]
    return min(PROJECT_XTOL, max(1.0e-12, 1000.0 * deviation))


# ---- C. finite differences around a caller's objective, beyond one lane trip (bit for bit with the fused run) -------------
# (objective, n, chains, axes per chunk or None for the default: one chunk of n axes)
FD_UNFUSED = (
    ("sphere", 33, 7, 20),            # the second trip of `ia += LPR` (20 > 16 lanes); axis0 = 20
    ("styblinski_tang", 65, 7, 33),   # 32-lane rows; chunks 33 + 32
    ("rastrigin", 130, 7, None),      # 64-lane rows, three trips over 130 axes
    ("sphere", 130, 40, 70),          # several workgroups; chunks 70 + 60
    ("styblinski_tang", 257, 3, 64),  # chunks 64 * 4 + 1
)
ANALYTIC_UNFUSED = (("griewank", 65, 7), ("ackley", 128, 40), ("rastrigin", 257, 7))


# ---- D. constraints="Reject" through one planted element ------------------------------------------------------------------
REJECT_CHAINS, REJECT_MAXITER, REJECT_SEED = 16, 8, 41
REJECT_PAIRS = ((17, 0), (17, 15), (17, 16), (65, 31), (65, 32), (65, 64), (129, 63), (129, 64), (129, 128), (257, 255),
                (257, 256), (600, 599))
REJECT_CASES = tuple((method, n, e) for method in ("mcmc", "hmc") for n, e in REJECT_PAIRS)
REJECT_TOTAL = REJECT_CHAINS * (REJECT_MAXITER - 1)
REJECT_MARGIN = 1.0e-12  # of the range: no proposal's planted element comes this close to its bound


def reject_x0(n, e):
    """Zeros (a hundred mcmc step sizes inside the box) but element e, which sits a billionth of its bound inside it, on
    alternating sides: a proposal leaves the box through element e or not at all."""
    x0 = np.zeros((REJECT_CHAINS, n))
    x0[:, e] = UPPER * (1.0 - 1.0e-9) * np.where(np.arange(REJECT_CHAINS) % 2 == 0, 1.0, -1.0)
    return x0


def reject_options(method):
    o = {"maxiter": REJECT_MAXITER, "seed": REJECT_SEED, "rng": "philox", "chains": REJECT_CHAINS, "constraints": "Reject",
         "return_all": True}
    o.update({"stepsize": 0.01, "perc": 1.0} if method == "mcmc" else {"stepsize": 0.002, "nleap": 2, "jac": "analytic"})
    return o


@functools.lru_cache(maxsize=None)
def reject_reference(case):
    """The restatement's run and its proposals (REJECT_MAXITER - 1, chains, n): every point the objective is asked for after
    the initial one (mcmc: the proposal; hmc with an analytic gradient: the end of the trajectory)."""
    method, n, e = case
    seen = []
    sphere = objectives.OBJECTIVES["sphere"]

    def recording(X):
        seen.append(np.array(X, copy=True))
        return sphere(X)

    objectives.OBJECTIVES["sphere"] = recording
    try:
        with np.errstate(all="ignore"):
            res = _sample_oracle.sample("sphere", bounds(n), x0=reject_x0(n, e), method=method, options=reject_options(method))
    finally:
        objectives.OBJECTIVES["sphere"] = sphere
    assert len(seen) == REJECT_MAXITER
    return res, np.stack(seen[1:])


# ---- E. mcmc at the layout edges ------------------------------------------------------------------------------------------
MCMC_NS = (1, 2, 16, 17, 32, 33, 64, 65, 129, 256, 257, 512, 1030)
MCMC_MAXITER, MCMC_STEP = 20, 0.05


def _mcmc_cases():
    out = []
    for k, n in enumerate(MCMC_NS):
        out.append((ALL[k % 7], n, (1.0, 0.5, 0.3)[k % 3], (1, 7, 40)[k % 3]))
    for k, n in enumerate(MCMC_NS[1:]):  # blocks of ONE variable
        out.append((ALL[(k + 3) % 7], n, 1.0 / n, (1, 7, 40)[(k + 1) % 3]))
    return tuple(out)


MCMC_CASES = _mcmc_cases()


def mcmc_id(case):
    name, n, perc, chains = case
    return f"{name}-{n}-perc{'1/n' if perc * n <= 1.0 + 1e-9 and n > 1 else perc}-{chains}"


def mcmc_options(case):
    name, n, perc, chains = case
    return {"maxiter": MCMC_MAXITER, "stepsize": MCMC_STEP, "perc": perc, "seed": 1234 + n + chains, "rng": "philox",
            "chains": chains, "return_all": True}


@functools.lru_cache(maxsize=None)
def mcmc_reference(case):
    name, n, _, _ = case
    with np.errstate(all="ignore"):
        return _sample_oracle.sample(name, bounds(n), method="mcmc", options=mcmc_options(case))


# ---- F. a cut run is the whole run, on wide rows --------------------------------------------------------------------------
CUT_NS = (130, 300)
CUT_MAXITER, CUT_FEW, CUT_MANY = 12, 7, 40
