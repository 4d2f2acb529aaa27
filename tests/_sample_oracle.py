"""numpy restatement of the two samplers (test infrastructure for tests/test_sample_host.py / test_gpu_sample.py).

Written from the behaviour the samplers are specified to have, with all chains advanced together as (C, ndim) arrays:

* mcmc: sample i perturbs block (i-1) mod ceil(ndim/k) of k = max(1, int(perc * ndim)) consecutive variables with
  randn(kb) * stepsize * 0.5 * (upper - lower), then draws one rand(); x / fun = best ACCEPTED sample (plain <).
* hmc: p = randn(ndim); half momentum step, position step, nleap x (momentum step, position step), half momentum
  step; d = U0 - U + K0 - K; one rand(); x / fun = argmin over funall; gradients by 2-point finite differences that
  perturb and restore x1[i], x2[i] in place, or the closed forms below (jac="analytic").
* acceptance: (d if d < 0 else 0.0) > log(u)  (Python's min(0.0, d): a NaN d gives 0.0).
* constraints="Reject": a proposal outside [lower, upper] is rejected without an acceptance draw (Philox mode only).

Draws: rng="numpy-legacy" consumes numpy's global stream in the reference's order (one chain); rng="philox" uses the
kernels' counter layout (slot, chain, sample, purpose) with the row layout of oracle/streams.py PhiloxStream: element e of
a row of ndim elements is lane l = e % LPR at step q = e // LPR (LPR = 16 / 32 / 64 lanes for ndim <= 64 / <= 128 / larger),
slot = (q >> 1) * LPR + l, half = q & 1.  Proposal normals purpose 10 (the normal of VARIABLE e, used when e is in the
sample's block), momentum normals 11 (Box-Muller of the call's two doubles: half 0 cosine, half 1 sine), acceptance
uniform 12 (slot 0, first double), initial point 13 (double `half` of the call).
"""
import numpy as np

from oracle import objectives
from oracle.streams import PhiloxStream, philox4x32_10, u53

PURPOSE_PROPOSAL, PURPOSE_MOMENTUM, PURPOSE_ACCEPT, PURPOSE_INIT = 10, 11, 12, 13
TWO_PI = 6.283185307179586


class Result(dict):
    __getattr__ = dict.__getitem__


# ---- closed-form gradients, rows of a (C, n) array ------------------------------------------------------------------
def grad_ackley(X):
    n = X.shape[1]
    r = np.sqrt(np.square(X).sum(axis=1, keepdims=True) / n)
    s2 = np.cos(TWO_PI * X).sum(axis=1, keepdims=True) / n
    with np.errstate(invalid="ignore", divide="ignore"):
        g1 = np.where(r > 0.0, 4.0 * np.exp(-0.2 * r) * X / (n * r), 0.0)
    return g1 + np.exp(s2) * TWO_PI * np.sin(TWO_PI * X) / n


def grad_griewank(X):
    s = np.sqrt(np.arange(1, X.shape[1] + 1))
    t = X / s
    prod = np.prod(np.cos(t), axis=1, keepdims=True)
    return X / 2000.0 + prod / np.cos(t) * np.sin(t) / s


def grad_quartic(X):
    return 4.0 * np.arange(1, X.shape[1] + 1) * X**3


def grad_rastrigin(X):
    return 2.0 * X + 10.0 * TWO_PI * np.sin(TWO_PI * X)


def grad_rosenbrock(X):
    g = np.zeros_like(X)
    g[:, :-1] += -400.0 * X[:, :-1] * (X[:, 1:] - X[:, :-1] ** 2) - 2.0 * (1.0 - X[:, :-1])
    g[:, 1:] += 200.0 * (X[:, 1:] - X[:, :-1] ** 2)
    return g


def grad_sphere(X):
    return 2.0 * X


def grad_styblinski_tang(X):
    return 0.5 * (4.0 * X**3 - 32.0 * X + 5.0)


GRADIENTS = {"ackley": grad_ackley, "griewank": grad_griewank, "quartic": grad_quartic, "rastrigin": grad_rastrigin,
             "rosenbrock": grad_rosenbrock, "sphere": grad_sphere, "styblinski_tang": grad_styblinski_tang}


# ---- draws ----------------------------------------------------------------------------------------------------------
class LegacyDraws:
    """numpy's global stream, consumed as the reference consumes it (one chain)."""

    def __init__(self, seed, chains, ndim):
        assert chains == 1
        if seed is not None:
            np.random.seed(seed)

    def initial(self, lower, upper):
        return np.random.uniform(lower, upper)[None, :]

    def normals(self, first, last, it, purpose):
        return np.random.randn(last - first)[None, :]

    def accept_uniform(self, it, feasible):
        return np.array([np.random.rand()])


class PhiloxDraws:
    def __init__(self, seed, chains, ndim):
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.k0, self.k1 = seed & 0xFFFFFFFF, seed >> 32
        self.rows = np.arange(chains, dtype=np.uint64)[:, None]
        q, lane = PhiloxStream._lanes(ndim)
        self.slot = ((q >> np.uint64(1)) * np.uint64(PhiloxStream.lanes_per_row(ndim)) + lane)[0]
        self.half = (q & np.uint64(1)).astype(bool)[0]

    def _call(self, slots, it, purpose):
        w = philox4x32_10(np.asarray(slots, dtype=np.uint64)[None, :], self.rows, it, purpose, self.k0, self.k1)
        return u53(w[0], w[1]), u53(w[2], w[3])

    def initial(self, lower, upper):
        d0, d1 = self._call(self.slot, 0, PURPOSE_INIT)
        return lower + (upper - lower) * np.where(self.half, d1, d0)

    def normals(self, first, last, it, purpose):
        """The normals of elements [first, last) of the row."""
        d0, d1 = self._call(self.slot[first:last], it, purpose)
        rad = np.sqrt(-2.0 * np.log(1.0 - d0))
        ang = TWO_PI * d1
        return np.where(self.half[first:last], rad * np.sin(ang), rad * np.cos(ang))

    def accept_uniform(self, it, feasible):
        return self._call([0], it, PURPOSE_ACCEPT)[0][:, 0]


def _log_accept(d, u):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d < 0.0, d, 0.0) > np.log(u)


def _in_box(Q, lower, upper):
    return np.all((Q >= lower) & (Q <= upper), axis=1)


def _numerical_gradient(f, Q, h, count):
    X1, X2 = Q.copy(), Q.copy()
    G = np.empty_like(Q)
    for i in range(Q.shape[1]):
        X1[:, i] -= h
        X2[:, i] += h
        G[:, i] = f(X2) - f(X1)
        X1[:, i] += h
        X2[:, i] -= h
    count[0] += 2 * Q.shape[1] * Q.shape[0]
    return 0.5 * G / h


def sample(fun, bounds, x0=None, method="mcmc", options=None, callback=None):
    """``fun`` is an objective's name.  Options as stochopy_amd.sample.sample (chains, rng included)."""
    o = dict(options or {})
    chains, rng = o.pop("chains", 1), o.pop("rng", "numpy-legacy")
    o.pop("backend", None)
    maxiter, seed = o.pop("maxiter", 100), o.pop("seed", None)
    constraints, return_all = o.pop("constraints", None), o.pop("return_all", True)
    mcmc = method == "mcmc"
    stepsize = o.pop("stepsize", 0.1 if mcmc else 0.01)
    if mcmc:
        perc = o.pop("perc", 1.0)
    else:
        nleap, jac, h = o.pop("nleap", 10), o.pop("jac", None), o.pop("finite_diff_abs_step", 1.0e-4)
    assert not o, f"unknown options {sorted(o)}"
    f = objectives.OBJECTIVES[fun]
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n, C = len(lower), chains
    step = np.full(n, stepsize, dtype=np.float64) if np.ndim(stepsize) == 0 else np.array(stepsize, dtype=np.float64)
    step = step * (0.5 * (upper - lower))
    if rng == "numpy-legacy":
        if constraints == "Reject" or C != 1:
            raise ValueError("numpy-legacy draws serve one chain without feasibility rejection")
        draws = LegacyDraws(seed, C, n)
    else:
        draws = PhiloxDraws(seed, C, n)
    reject = constraints == "Reject"

    xall = np.empty((C, maxiter, n))
    funall = np.empty((C, maxiter))
    xall[:, 0] = np.broadcast_to(np.asarray(x0, dtype=np.float64), (C, n)) if x0 is not None else draws.initial(lower, upper)
    funall[:, 0] = f(xall[:, 0])
    nfev = [C]
    nacc = np.zeros(C, dtype=np.int64)
    nfeas = np.zeros(C, dtype=np.int64)
    imin = np.zeros(C, dtype=np.int64)  # best ACCEPTED sample
    fmin = np.full(C, np.inf)
    rows = np.arange(C)

    def squeeze(a):
        return a[0] if C == 1 else a

    def call_back(i):
        if callback is None:
            return
        fnow = funall[rows, imin]
        b = int(np.argmin(fnow))
        state = Result(x=xall[b, imin[b]], fun=fnow[b], nit=i + 1,
                       accept_ratio=1.0 if i == 0 else int(nacc.sum()) / (C * (i + 1)))
        if return_all:
            state["xall"], state["funall"] = squeeze(xall[:, :max(i, 1)]), squeeze(funall[:, :max(i, 1)])
        callback(squeeze(xall[:, i]), state)

    call_back(0)
    if mcmc:
        k = max(1, int(perc * n))
        nblocks = -(-n // k)
    for i in range(1, maxiter):
        cur, fcur = xall[:, i - 1], funall[:, i - 1]
        if mcmc:
            j0 = ((i - 1) % nblocks) * k
            j1 = min(n, j0 + k)
            prop = cur.copy()
            prop[:, j0:j1] += draws.normals(j0, j1, i, PURPOSE_PROPOSAL) * step[j0:j1]
            with np.errstate(invalid="ignore", over="ignore"):
                fprop = f(prop)
                d = fcur - fprop
        else:
            if jac == "analytic":
                grad = GRADIENTS[fun]
            else:
                grad = lambda Q: _numerical_gradient(f, Q, h, nfev)  # noqa: E731
            q = cur.copy()
            p = np.array(np.broadcast_to(draws.normals(0, n, i, PURPOSE_MOMENTUM), (C, n)))
            p0 = p.copy()
            with np.errstate(invalid="ignore", over="ignore"):
                p -= 0.5 * step * grad(q)
                q += step * p
                for _ in range(nleap):
                    p -= step * grad(q)
                    q += step * p
                p -= 0.5 * step * grad(q)
                prop, fprop = q, f(q)
                K0 = 0.5 * np.square(p0).sum(axis=1)
                K = 0.5 * np.square(p).sum(axis=1)
                d = fcur - fprop + K0 - K
        feasible = _in_box(prop, lower, upper) if reject else np.ones(C, dtype=bool)
        if not mcmc:
            nfev[0] += 2 * int(feasible.sum())
        nfeas += feasible
        accept = feasible & _log_accept(d, draws.accept_uniform(i, feasible))
        nacc += accept
        xall[:, i] = np.where(accept[:, None], prop, cur)
        funall[:, i] = np.where(accept, fprop, fcur)
        better = accept & (fprop < fmin)
        imin[better] = i
        fmin[better] = fprop[better]
        call_back(i)

    if mcmc:
        per_f, per_i = fmin, imin
    else:
        per_i = np.array([int(np.argmin(funall[c])) for c in range(C)])
        per_f = funall[rows, per_i]
    b = int(np.argmin(per_f))
    res = Result(x=xall[b, per_i[b]], fun=per_f[b], nit=maxiter, accept_ratio=int(nacc.sum()) / (C * maxiter),
                 nacc=nacc, nfeas=nfeas)
    if not mcmc:
        res["nfev"] = nfev[0]
    if C > 1:
        res["accept_ratios"] = nacc / maxiter
    if return_all:
        res["xall"], res["funall"] = squeeze(xall), squeeze(funall)
    return res
