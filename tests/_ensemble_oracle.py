"""numpy restatement of the affine-invariant ensemble sampler, method="ensemble" (test infrastructure for
tests/test_sample_ensemble_host.py / test_gpu_sample_ensemble.py), all C * W walkers advanced together as arrays.

Built on tests/_sample_oracle.py (PhiloxDraws, _log_accept, _in_box, the oracle objectives).  C ensembles of W walkers, W even,
>= 4 and >= 2 ndim, h = W / 2; walker w of ensemble g is replica q = g W + w, which takes the chain index's place in every draw.
Sample 0 is the initial state (x0=None: every replica's own uniform point in the box; (W, ndim) shared by all ensembles, or
(C, W, ndim)).  Sample it >= 1 is two half-sweeps: in half 0 the walkers w < h are active and read the walkers [h, W), in half 1
the walkers w >= h are active and read [0, h), already updated.  The active walker q makes one Philox call (slot 0, row q,
sample it, purpose 15) with doubles (d0, d1):
    j = base + min(h - 1, int(d0 * h)), base the first walker of the other half;   z = ((a - 1) * d1 + 1)^2 / a
    Y = X_j + z * (X_q - X_j);   d = (ndim - 1) * log(z) + (fcur_q - f(Y));   accepted when (d if d < 0 else 0.0) > log(u)
u the acceptance draw of (q, it), purpose 12.  constraints="Reject": a Y outside [lower, upper] is rejected without that draw and
nfeas counts the feasible ones.  x / fun: the best ACCEPTED sample over all walkers (plain <; fun = inf and x = walker 0's first
sample when nothing was accepted).
"""
import numpy as np

import _sample_oracle as so
from oracle import objectives

PURPOSE_STRETCH = 15


def sample(fun, bounds, x0=None, options=None, callback=None, on_half=None):
    """``fun``: an objective's name, or a callable on (P, n) arrays.  Options as stochopy_amd.sample.sample with
    method="ensemble" (chains = ensembles; walkers; stretch).  ``on_half(it, half, X)``: called after each half-sweep with the
    (C, W, n) states."""
    o = dict(options or {})
    C, maxiter, seed = o.pop("chains", 1), o.pop("maxiter", 100), o.pop("seed", None)
    assert o.pop("rng", "philox") == "philox"
    o.pop("backend", None)
    constraints, return_all = o.pop("constraints", None), o.pop("return_all", True)
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    W, a = o.pop("walkers", None), float(o.pop("stretch", 2.0))
    assert not o, f"unknown options {sorted(o)}"
    W = max(4, 2 * n) if W is None else W
    assert W % 2 == 0 and W >= 4 and W >= 2 * n and a > 1.0
    f = objectives.OBJECTIVES[fun] if isinstance(fun, str) else fun
    h, R = W // 2, C * W
    draws = so.PhiloxDraws(seed, R, n)
    reject = constraints == "Reject"
    first = (np.arange(C) * W)[:, None]  # the first replica of each ensemble

    if x0 is None:
        X = draws.initial(lower, upper)
    else:
        x0 = np.asarray(x0, dtype=np.float64)
        assert x0.shape in ((W, n), (C, W, n))
        X = np.tile(x0, (C, 1)) if x0.ndim == 2 else x0.reshape(R, n)
    X = np.array(X, dtype=np.float64)
    with np.errstate(all="ignore"):
        fcur = np.array(f(X), dtype=np.float64)
    xall = np.empty((C, maxiter, W, n))
    funall = np.empty((C, maxiter, W))
    nacc, nfeas = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64)
    facc, iacc, xbest = np.full(R, np.inf), np.zeros(R, dtype=np.int64), X.copy()

    def squeeze(v):
        return v[0] if C == 1 else v

    def record(i):
        xall[:, i], funall[:, i] = X.reshape(C, W, n), fcur.reshape(C, W)
        if callback is not None:
            fnow = np.where(iacc == 0, funall[:, 0].reshape(R), facc)
            b = int(np.argmin(fnow))
            state = so.Result(x=xbest[b].copy(), fun=fnow[b], nit=i + 1,
                              accept_ratio=1.0 if i == 0 else int(nacc.sum()) / (R * (i + 1)))
            if return_all:
                state["xall"], state["funall"] = squeeze(xall[:, :max(i, 1)]), squeeze(funall[:, :max(i, 1)])
            callback(squeeze(xall[:, i]).copy(), state)

    record(0)
    for it in range(1, maxiter):
        d0, d1 = (v[:, 0] for v in draws._call([0], it, PURPOSE_STRETCH))
        u = draws.accept_uniform(it, None)
        for half in (0, 1):
            act = (first + half * h + np.arange(h)[None, :]).ravel()  # the active replicas
            jj = np.minimum(h - 1, (d0[act] * h).astype(np.int64))
            j = (act // W) * W + (h - half * h) + jj
            t = (a - 1.0) * d1[act] + 1.0
            z = (t * t) / a
            Y = X[j] + z[:, None] * (X[act] - X[j])
            with np.errstate(all="ignore"):
                fY = np.array(f(Y), dtype=np.float64)
                d = float(n - 1) * np.log(z) + (fcur[act] - fY)
            feasible = so._in_box(Y, lower, upper) if reject else np.ones(act.size, dtype=bool)
            nfeas[act] += feasible
            accept = feasible & so._log_accept(d, u[act])
            nacc[act] += accept
            won = act[accept]
            X[won], fcur[won] = Y[accept], fY[accept]
            better = accept & (fY < facc[act])
            facc[act[better]], iacc[act[better]], xbest[act[better]] = fY[better], it, Y[better]
            if on_half is not None:
                on_half(it, half, X.reshape(C, W, n).copy())
        record(it)

    b = int(np.argmin(facc))
    res = so.Result(x=xbest[b], fun=facc[b], nit=maxiter, accept_ratio=int(nacc.sum()) / (R * maxiter),
                    nacc=nacc.reshape(C, W), nfeas=nfeas.reshape(C, W), accept_ratios=nacc.reshape(C, W) / maxiter,
                    walkers=W, stretch=a)
    if reject:
        res["nreject"] = R * (maxiter - 1) - int(nfeas.sum())
    if return_all:
        res["xall"], res["funall"] = squeeze(xall), squeeze(funall)
    return res
