"""numpy restatement of the tempered Metropolis-Hastings run (test infrastructure for tests/test_sample_temper_host.py /
test_gpu_sample_temper.py), all C * K replicas advanced together as (C K, ndim) arrays.

Built on tests/_sample_oracle.py (PhiloxDraws, _log_accept, _in_box, the oracle objectives), whose mcmc sample it repeats
with d = (fcur - fprop) * beta[rung]; replica q = c K + k is rung k of ladder c and takes the chain index's place in every
draw.  After sample it >= 1 with it % swap_every == 0 the exchange event j = it // swap_every pairs rungs (0,1), (2,3), ...
(odd j) or (1,2), (3,4), ... (even j); the pair (k, k+1) exchanges its states (X and fcur) when
(d if d < 0 else 0.0) > log(u), d = (beta[k] - beta[k+1]) * (f_k - f_{k+1}), u = first double of the Philox call
(slot 0, row = the LOWER rung's replica, sample it, purpose 14).  Sample `it` of a replica is its state after the event.
An exchange is no proposal (nacc, nfeas stay); an arriving state is compared with the replica's best accepted value as
an accepted proposal of sample `it` is.
"""
import numpy as np

import _sample_oracle as so
from oracle import objectives

PURPOSE_SWAP = 14


def swap_attempts(K, maxiter, swap_every):
    J = (maxiter - 1) // swap_every
    return np.array([sum(1 for j in range(1, J + 1) if (j + 1) % 2 == k % 2) for k in range(K - 1)], dtype=np.int64)


def sample(fun, bounds, temperatures, x0=None, options=None, callback=None, keep_hot=False):
    """``fun``: an objective's name, or a callable on (P, n) arrays.  Options as stochopy_amd.sample.sample with
    method="mcmc" (chains = ladders; swap_every).  ``keep_hot``: xall_replicas (C K, maxiter, n) as well."""
    o = dict(options or {})
    C, maxiter, seed = o.pop("chains", 1), o.pop("maxiter", 100), o.pop("seed", None)
    assert o.pop("rng", "philox") == "philox"
    o.pop("backend", None)
    constraints, return_all = o.pop("constraints", None), o.pop("return_all", True)
    stepsize, perc, every = o.pop("stepsize", 0.1), o.pop("perc", 1.0), o.pop("swap_every", 1)
    assert not o, f"unknown options {sorted(o)}"
    f = objectives.OBJECTIVES[fun] if isinstance(fun, str) else fun
    T = np.asarray(temperatures, dtype=np.float64)
    beta = 1.0 / T
    K = T.size
    R = C * K
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    step = np.full(n, stepsize, dtype=np.float64) if np.ndim(stepsize) == 0 else np.array(stepsize, dtype=np.float64)
    step = step * (0.5 * (upper - lower))
    draws = so.PhiloxDraws(seed, R, n)
    reject = constraints == "Reject"
    rung = np.arange(R) % K
    brow = beta[rung]
    cold = np.arange(C) * K

    if x0 is None:
        X = draws.initial(lower, upper)
    else:
        x0 = np.asarray(x0, dtype=np.float64)
        X = np.repeat(x0, K, axis=0) if x0.ndim == 2 else np.broadcast_to(x0, (R, n)).copy()
    X = np.array(X, dtype=np.float64)
    with np.errstate(all="ignore"):
        fcur = np.array(f(X), dtype=np.float64)
    xall = np.empty((C, maxiter, n))
    funall = np.empty((C, maxiter))
    hot = np.empty((R, maxiter, n)) if keep_hot else None
    nacc, nfeas, nswap = (np.zeros(R, dtype=np.int64) for _ in range(3))
    facc, iacc, xbest = np.full(R, np.inf), np.zeros(R, dtype=np.int64), X.copy()
    k = max(1, int(perc * n))
    nblocks = -(-n // k)

    def squeeze(a):
        return a[0] if C == 1 else a

    def record(i):
        xall[:, i], funall[:, i] = X[cold], fcur[cold]
        if keep_hot:
            hot[:, i] = X
        if callback is not None:
            fnow = np.where(iacc[cold] == 0, funall[:, 0], facc[cold])
            b = int(np.argmin(fnow))
            state = so.Result(x=xbest[cold][b].copy(), fun=fnow[b], nit=i + 1,
                              accept_ratio=1.0 if i == 0 else int(nacc[cold].sum()) / (C * (i + 1)))
            if return_all:
                state["xall"], state["funall"] = squeeze(xall[:, :max(i, 1)]), squeeze(funall[:, :max(i, 1)])
            callback(squeeze(xall[:, i]).copy(), state)

    record(0)
    for i in range(1, maxiter):
        j0 = ((i - 1) % nblocks) * k
        j1 = min(n, j0 + k)
        prop = X.copy()
        prop[:, j0:j1] += draws.normals(j0, j1, i, so.PURPOSE_PROPOSAL) * step[j0:j1]
        with np.errstate(all="ignore"):
            fprop = np.array(f(prop), dtype=np.float64)
            d = (fcur - fprop) * brow
        feasible = so._in_box(prop, lower, upper) if reject else np.ones(R, dtype=bool)
        nfeas += feasible
        accept = feasible & so._log_accept(d, draws.accept_uniform(i, feasible))
        nacc += accept
        X = np.where(accept[:, None], prop, X)
        fcur = np.where(accept, fprop, fcur)
        better = accept & (fprop < facc)
        facc[better], iacc[better], xbest[better] = fprop[better], i, prop[better]
        if i % every == 0:
            j = i // every
            lo = np.nonzero((rung % 2 == (j + 1) % 2) & (rung + 1 < K))[0]  # the lower rungs' replicas
            if lo.size:
                u = draws._call([0], i, PURPOSE_SWAP)[0][:, 0][lo]
                with np.errstate(all="ignore"):
                    ds = (beta[rung[lo]] - beta[rung[lo] + 1]) * (fcur[lo] - fcur[lo + 1])
                ql = lo[so._log_accept(ds, u)]
                qu = ql + 1
                nswap[ql] += 1
                X[ql], X[qu] = X[qu].copy(), X[ql].copy()
                fcur[ql], fcur[qu] = fcur[qu].copy(), fcur[ql].copy()
                for q in (ql, qu):
                    bet = q[fcur[q] < facc[q]]
                    facc[bet], iacc[bet], xbest[bet] = fcur[bet], i, X[bet]
        record(i)

    b = int(np.argmin(facc[cold]))
    attempts = swap_attempts(K, maxiter, every)
    swaps = nswap.reshape(C, K)[:, :K - 1]
    res = so.Result(x=xbest[cold][b], fun=facc[cold][b], nit=maxiter, accept_ratio=int(nacc[cold].sum()) / (C * maxiter),
                    nacc=nacc.reshape(C, K), nfeas=nfeas.reshape(C, K), nswap=swaps, accept_ratios=nacc.reshape(C, K) / maxiter,
                    temperatures=T, swap_ratios=np.where(attempts > 0, swaps / np.maximum(attempts, 1), 0.0))
    if reject:
        res["nreject"] = C * (maxiter - 1) - int(nfeas[cold].sum())
    if return_all:
        res["xall"], res["funall"] = squeeze(xall), squeeze(funall)
    if keep_hot:
        res["xall_replicas"] = hot
    return res
