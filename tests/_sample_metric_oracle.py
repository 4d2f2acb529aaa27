"""numpy restatement of the samplers with per-axis scale adaptation in the warm-up (metric="diag"; test infrastructure for
tests/test_sample_metric_host.py / test_gpu_sample_metric.py; Philox draws only).

Written from the rule, not from the kernels.  On top of tests/_sample_adapt_oracle.py (whose docstring states the dual
averaging): chain c carries m_c[e] (1.0 at the start) and eff_c[e] = m_c[e] * step[e], and every place that read
s_c * step[e] reads s_c * eff_c[e].  Windows (b_0, b_1], (b_1, b_2], ... (b_{J-1}, b_J] lie inside the warm-up.  After the
decision of sample it with b_{j-1} < it <= b_j, x the chain's state and N = it - b_{j-1}, per element

    delta = x - mean;   mean += delta / N;   M2 += delta * (x - mean)

and at it == b_j, after that and after the sample's step of the dual averaging, with h = 0.5 * (upper - lower):

    var = M2 / (N - 1);   v = (N / (N + 5)) * var + ((5 / (N + 5)) * 1e-3) * (h * h);   r = sqrt(v)
    m = r / exp(sum(log r) / n);   eff = m * step          unless some r is not finite or not positive: the chain keeps m
    mean = M2 = 0
    sbase = sbase * exp(logsbar);   hbar = logsbar = 0;   s = sbase;   the clock of the dual averaging restarts at b_j

While adapting s = sbase * exp(logs) with t = float(it - the last window end before it), at it == W s = sbase * exp(logsbar).
Without windows sbase = 1.0 and t = float(it): tests/_sample_adapt_oracle.py, bit for bit.
"""
import numpy as np

from oracle import objectives

import _sample_adapt_oracle
from _sample_adapt_oracle import GAMMA, LOG_MU, T0, default_target
from _sample_oracle import (GRADIENTS, PURPOSE_MOMENTUM, PURPOSE_PROPOSAL, PhiloxDraws, Result, _in_box, _log_accept,
                            _numerical_gradient)

__all__ = ["sample", "windows", "GRADIENTS", "default_target"]
assert _sample_adapt_oracle  # (its constants are this rule's)


def windows(W):
    """(b_0, (b_1, ..., b_J)) of a warm-up of W >= 20 samples: 15 % in front, 10 % behind, doubling windows between."""
    start, end = (15 * W) // 100, W - (10 * W) // 100
    span = end - start
    J = max(j for j in (1, 2, 3, 4) if span // (2 ** j - 1) >= 8)
    first = span // (2 ** J - 1)
    ends = [start + first * (2 ** j - 1) for j in range(1, J)] + [end]
    return start, tuple(ends)


def sample(fun, bounds, x0=None, method="mcmc", options=None):
    """``fun`` is an objective's name, or a callable on (C, n) rows (then ``jac`` is None or a callable too).  Options as
    tests/_sample_adapt_oracle.py's, and ``metric`` (None | "diag": the schedule above) or ``windows`` ((b_0, ends), placed
    freely; () ends: none)."""
    o = dict(options or {})
    C, maxiter, seed = o.pop("chains", 1), o.pop("maxiter", 100), o.pop("seed", None)
    assert o.pop("rng", "philox") == "philox"
    o.pop("backend", None)
    reject = o.pop("constraints", None) == "Reject"
    W, target, B, T = o.pop("warmup", 0), o.pop("target_accept", None), o.pop("burn", None), o.pop("thin", 1)
    B = W if B is None else B
    metric, win = o.pop("metric", None), o.pop("windows", None)
    if win is None:
        win = windows(W) if metric == "diag" else (0, ())
    b0, ends = int(win[0]), [int(b) for b in win[1]]
    edges = [b0] + ends
    assert all(lo < hi for lo, hi in zip(edges, edges[1:])) and (not ends or ends[-1] <= W)
    mcmc = method == "mcmc"
    stepsize = o.pop("stepsize", 0.1 if mcmc else 0.01)
    if mcmc:
        perc = o.pop("perc", 1.0)
    else:
        nleap, jac, h = o.pop("nleap", 10), o.pop("jac", None), o.pop("finite_diff_abs_step", 1.0e-4)
    assert not o, f"unknown options {sorted(o)}"
    named = isinstance(fun, str)

    def f(X):  # (looked up per call: tools/sample_metric_sensitivity.py swaps the table's entries)
        return objectives.OBJECTIVES[fun](X) if named else fun(X)

    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    step = np.full(n, stepsize, dtype=np.float64) if np.ndim(stepsize) == 0 else np.array(stepsize, dtype=np.float64)
    half = 0.5 * (upper - lower)
    step = step * half
    draws = PhiloxDraws(seed, C, n)
    k = max(1, int(perc * n)) if mcmc else n
    nblocks = -(-n // k)
    if target is None:
        target = default_target(method, k)

    xall = np.empty((C, maxiter, n))
    funall = np.empty((C, maxiter))
    xall[:, 0] = np.broadcast_to(np.asarray(x0, dtype=np.float64), (C, n)) if x0 is not None else draws.initial(lower, upper)
    funall[:, 0] = f(xall[:, 0])
    nfev = [C]
    nacc, nfeas, nacc_warm = (np.zeros(C, dtype=np.int64) for _ in range(3))
    imin, fmin = np.zeros(C, dtype=np.int64), np.full(C, np.inf)  # best ACCEPTED sample
    s, hbar, logsbar, sbase = np.ones(C), np.zeros(C), np.zeros(C), np.ones(C)
    m, mean, M2 = np.ones((C, n)), np.zeros((C, n)), np.zeros((C, n))
    eff = m * step
    rows = np.arange(C)
    with np.errstate(all="ignore"):
        for i in range(1, maxiter):
            cur, fcur = xall[:, i - 1], funall[:, i - 1]
            eps = s[:, None] * eff  # (C, n): the step of every chain, formed first
            if mcmc:
                j0 = ((i - 1) % nblocks) * k
                j1 = min(n, j0 + k)
                prop = cur.copy()
                prop[:, j0:j1] += draws.normals(j0, j1, i, PURPOSE_PROPOSAL) * eps[:, j0:j1]
                fprop = f(prop)
                d = fcur - fprop
            else:
                if jac == "analytic":
                    grad = lambda Q: GRADIENTS[fun](Q)  # noqa: E731
                elif jac is None:
                    grad = lambda Q: _numerical_gradient(f, Q, h, nfev)  # noqa: E731
                else:
                    grad = jac
                q = cur.copy()
                p = np.array(np.broadcast_to(draws.normals(0, n, i, PURPOSE_MOMENTUM), (C, n)))
                p0 = p.copy()
                p -= 0.5 * eps * grad(q)
                q += eps * p
                for _ in range(nleap):
                    p -= eps * grad(q)
                    q += eps * p
                p -= 0.5 * eps * grad(q)
                prop, fprop = q, f(q)
                d = fcur - fprop + 0.5 * np.square(p0).sum(axis=1) - 0.5 * np.square(p).sum(axis=1)
            feasible = _in_box(prop, lower, upper) if reject else np.ones(C, dtype=bool)
            if not mcmc:
                nfev[0] += 2 * int(feasible.sum())
            nfeas += feasible
            accept = feasible & _log_accept(d, draws.accept_uniform(i, feasible))
            nacc += accept
            xall[:, i] = np.where(accept[:, None], prop, cur)
            funall[:, i] = np.where(accept, fprop, fcur)
            better = accept & (fprop < fmin)
            imin[better], fmin[better] = i, fprop[better]
            window = [j for j in range(len(ends)) if edges[j] < i <= edges[j + 1]]
            if window:
                N = float(i - edges[window[0]])
                x = xall[:, i]
                delta = x - mean
                mean = mean + delta / N
                M2 = M2 + delta * (x - mean)
            if i <= W:
                t = float(i - max([b for b in ends if b < i], default=0))
                alpha = np.where(~feasible, 0.0, np.where(d < 0.0, np.exp(np.where(d < 0.0, d, 0.0)), np.where(d >= 0.0, 1.0, 0.0)))
                eta = 1.0 / (t + T0)
                hbar = (1.0 - eta) * hbar + eta * (target - alpha)
                logs = LOG_MU - (np.sqrt(t) / GAMMA) * hbar
                w = 1.0 / (np.sqrt(t) * np.sqrt(np.sqrt(t)))
                logsbar = w * logs + (1.0 - w) * logsbar
                s = sbase * (np.exp(logs) if i < W else np.exp(logsbar))
                if i == W:
                    nacc_warm = nacc.copy()
            if window and i == edges[window[0] + 1]:
                var = M2 / (N - 1.0)
                v = (N / (N + 5.0)) * var + ((5.0 / (N + 5.0)) * 1.0e-3) * (half * half)
                r = np.sqrt(v)
                ok = np.all(np.isfinite(r) & (r > 0.0), axis=1)
                new = r / np.exp(np.log(r).sum(axis=1) / n)[:, None]
                m = np.where(ok[:, None], new, m)
                eff = m * step
                mean, M2 = np.zeros((C, n)), np.zeros((C, n))
                sbase = sbase * np.exp(logsbar)
                hbar, logsbar = np.zeros(C), np.zeros(C)
                s = sbase.copy()

    if mcmc:
        per_f, per_i = fmin, imin
    else:
        per_i = np.array([int(np.argmin(funall[c])) for c in range(C)])
        per_f = funall[rows, per_i]
    b = int(np.argmin(per_f))

    def squeeze(a):
        return a[0] if C == 1 else a

    after = maxiter - 1 - W
    res = Result(x=xall[b, per_i[b]], fun=per_f[b], nit=maxiter, accept_ratio=int(nacc.sum()) / (C * maxiter),
                 nacc=nacc, nfeas=nfeas, nacc_warm=nacc_warm, accept_ratios=nacc / maxiter,
                 xall=squeeze(xall[:, B::T]), funall=squeeze(funall[:, B::T]), xall_full=xall, funall_full=funall)
    if not mcmc:
        res["nfev"] = nfev[0]
    if W > 0:
        res["stepsizes"] = squeeze(s)
        res["accept_ratios_sampling"] = squeeze((nacc - nacc_warm) / after if after > 0 else np.zeros(C))
        res["warmup"] = W
    if ends:
        res["metric"] = squeeze(m)
        res["metric_windows"] = tuple(ends)
    return res
