"""numpy restatement of the ensemble sampler with several moves, a burn-in and thinning, method="ensemble" with ``moves`` /
``burn`` / ``thin`` (test infrastructure for tests/test_sample_ensemble_moves_host.py / test_gpu_sample_ensemble_moves.py).

Built on tests/_sample_oracle.py (PhiloxDraws, _log_accept, _in_box) as tests/_ensemble_oracle.py is, and the same run but for
the proposal of sample it >= 1.  Ensemble g uses ONE entry (name, weight, param) in both half-sweeps of the sample: with u the
first double of Philox (slot 0, row g W, sample it, purpose 16) the first k with cum[k] > u, else the last; cum the running sums
of weight / sum(weights) with its last value set to 1.0 (one entry: no draw).
    "stretch", param a:  tests/_ensemble_oracle.py's proposal (purpose 15)
The other two draw (d0, d1) from slot 0 and (d2, d3) from slot 1 (row q, sample it, purpose 17) and pick distinct walkers of the
other half by their indices in it:  j1 = min(h - 1, int(d0 h));  j2 = min(h - 2, int(d1 (h - 1)));  j2 += (j2 >= j1)
    "de", param g0:      g = g0 * (1 + 1e-5 * (2 d2 - 1));  Y = X_q + g * (X_j1 - X_j2);  d = fcur_q - f(Y)
    "snooker", param gs: j3 = min(h - 3, int(d2 (h - 2)));  j3 += (j3 >= min(j1, j2));  j3 += (j3 >= max(j1, j2))
                         delta = X_q - X_j1;  dd = sum delta^2;  pr = sum delta * (X_j2 - X_j3)      (row_sum's order, below)
                         c = gs * (pr / dd), 0 where dd is not > 0 or c is not finite;  Y = X_q + c * delta
                         d = (n - 1) * log|1 + c| + (fcur_q - f(Y))
burn = B, thin = T: xall / funall hold samples B, B + T, ...; the counts and the best values run over all samples.
"""
import numpy as np

import _sample_oracle as so
from _ensemble_oracle import PURPOSE_STRETCH
from oracle import objectives
from oracle.streams import PhiloxStream

PURPOSE_MOVE, PURPOSE_DONORS = 16, 17
NAMES = ("stretch", "de", "snooker")


def checked_moves(moves, n, stretch=2.0):
    """[(name, normalised weight, param)] and cum, from a name or a sequence of name / (name, weight) / (name, weight, param)."""
    entries = [moves] if isinstance(moves, str) else list(moves)
    assert 1 <= len(entries) <= 4
    out = []
    for entry in entries:
        entry = (entry,) if isinstance(entry, str) else tuple(entry)
        name = entry[0]
        weight = float(entry[1]) if len(entry) > 1 else 1.0
        default = {"stretch": float(stretch), "de": 2.38 / np.sqrt(2.0 * n), "snooker": 1.7}[name]
        param = float(entry[2]) if len(entry) > 2 and entry[2] is not None else float(default)
        assert weight > 0.0 and (param > 1.0 if name == "stretch" else param > 0.0)
        out.append((name, weight, param))
    w = np.array([e[1] for e in out], dtype=np.float64)
    p = w / w.sum()
    cum = np.cumsum(p)
    cum[-1] = 1.0
    assert np.all(np.diff(np.concatenate(([0.0], cum))) > 0.0)
    return [(e[0], float(pk), e[2]) for e, pk in zip(out, p)], cum


def row_sum(T):
    """The sum of each row of T (P, n) in the order of the kernels' row_sum: lane l of the row's LPR lanes adds the terms
    l, l + LPR, ... in that order, then v += v[lane ^ 1], ^ 2, ^ 4, ... up to LPR / 2."""
    P, n = T.shape
    lpr = PhiloxStream.lanes_per_row(n)
    steps = -(-n // lpr)
    padded = np.zeros((P, steps * lpr))
    padded[:, :n] = T
    padded = padded.reshape(P, steps, lpr)
    v = np.zeros((P, lpr))
    for q in range(steps):
        v = v + padded[:, q, :]
    lane = np.arange(lpr)
    off = 1
    while off < lpr:
        v = v + v[:, lane ^ off]
        off <<= 1
    return v[:, 0]


def partners(d0, d1, d2, h, three):
    """The indices (j1, j2, j3) within the other half; j3 only with ``three`` (h >= 3), else zeros."""
    j1 = np.minimum(h - 1, (d0 * h).astype(np.int64))
    j2 = np.minimum(h - 2, (d1 * (h - 1)).astype(np.int64))
    j2 = j2 + (j2 >= j1)
    j3 = np.zeros_like(j1)
    if three:
        j3 = np.minimum(h - 3, (d2 * (h - 2)).astype(np.int64))
        j3 = j3 + (j3 >= np.minimum(j1, j2))
        j3 = j3 + (j3 >= np.maximum(j1, j2))
    return j1, j2, j3


def sample(fun, bounds, x0=None, options=None, callback=None, on_half=None, nudge=None):
    """``fun``: an objective's name, or a callable on (P, n) arrays.  Options as stochopy_amd.sample.sample with
    method="ensemble" (chains = ensembles; walkers; stretch; moves; burn; thin).  ``on_half(it, half, X)``: called after each
    half-sweep with the (C, W, n) states.  ``nudge(v)``: applied to the snooker move's dd and pr (the admission of seeds moves
    them by one unit in the last place).  The result also carries ``kinds (C, maxiter)``, the entry each ensemble used."""
    o = dict(options or {})
    C, maxiter, seed = o.pop("chains", 1), o.pop("maxiter", 100), o.pop("seed", None)
    assert o.pop("rng", "philox") == "philox"
    o.pop("backend", None)
    constraints, return_all = o.pop("constraints", None), o.pop("return_all", True)
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    W, a = o.pop("walkers", None), float(o.pop("stretch", 2.0))
    moves, burn, thin = o.pop("moves", None), o.pop("burn", 0), o.pop("thin", 1)
    assert not o, f"unknown options {sorted(o)}"
    W = max(4, 2 * n) if W is None else W
    assert W % 2 == 0 and W >= 4 and W >= 2 * n and a > 1.0
    assert 0 <= burn <= maxiter - 1 and thin >= 1
    given = moves is not None or burn != 0 or thin != 1
    entries, cum = checked_moves("stretch" if moves is None else moves, n, a)
    kind_of = np.array([NAMES.index(e[0]) for e in entries])
    param_of = np.array([e[2] for e in entries])
    any_snooker = bool(np.any(kind_of == 2))
    assert not any_snooker or W >= 6
    f = objectives.OBJECTIVES[fun] if isinstance(fun, str) else fun
    h, R = W // 2, C * W
    draws = so.PhiloxDraws(seed, R, n)
    reject = constraints == "Reject"
    first = (np.arange(C) * W)[:, None]  # the first replica of each ensemble
    recorded = np.arange(burn, maxiter, thin)

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
    kinds = np.full((C, maxiter), -1)

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
                upto = recorded[recorded < max(i, 1)]  # the recorded rows among the samples before the newest
                state["xall"], state["funall"] = squeeze(xall[:, upto]), squeeze(funall[:, upto])
            callback(squeeze(xall[:, i]).copy(), state)

    record(0)
    for it in range(1, maxiter):
        if len(entries) == 1:
            entry = np.zeros(C, dtype=np.int64)
        else:
            um = draws._call([0], it, PURPOSE_MOVE)[0][first[:, 0], 0]
            entry = np.minimum((cum[None, :] > um[:, None]).argmax(axis=1), len(entries) - 1)
            entry = np.where((cum[None, :] > um[:, None]).any(axis=1), entry, len(entries) - 1)
        kinds[:, it] = entry
        s0, s1 = (v[:, 0] for v in draws._call([0], it, PURPOSE_STRETCH))
        A, B = draws._call([0, 1], it, PURPOSE_DONORS)
        d0, d1, d2 = A[:, 0], B[:, 0], A[:, 1]
        u = draws.accept_uniform(it, None)
        for half in (0, 1):
            act = (first + half * h + np.arange(h)[None, :]).ravel()  # the active replicas
            other = (act // W) * W + (h - half * h)                   # the first walker of the other half
            kind = kind_of[entry][act // W]
            param = param_of[entry][act // W]
            with np.errstate(all="ignore"):
                # "stretch"
                jj = np.minimum(h - 1, (s0[act] * h).astype(np.int64))
                t = (param - 1.0) * s1[act] + 1.0
                z = (t * t) / param
                Xj = X[other + jj]
                Y = Xj + z[:, None] * (X[act] - Xj)
                factor = float(n - 1) * np.log(z)
                # "de"
                j1, j2, j3 = partners(d0[act], d1[act], d2[act], h, any_snooker)
                gamma = param * (1.0 + 1e-5 * (2.0 * d2[act] - 1.0))
                Yde = X[act] + gamma[:, None] * (X[other + j1] - X[other + j2])
                de = kind == 1
                Y[de], factor[de] = Yde[de], 0.0
                if any_snooker:
                    delta = X[act] - X[other + j1]
                    dd, pr = row_sum(delta * delta), row_sum(delta * (X[other + j2] - X[other + j3]))
                    if nudge is not None:
                        dd, pr = nudge(dd), nudge(pr)
                    c = param * (pr / dd)
                    c = np.where((dd > 0.0) & np.isfinite(c), c, 0.0)
                    Ysn = X[act] + c[:, None] * delta
                    sn = kind == 2
                    Y[sn], factor[sn] = Ysn[sn], (float(n - 1) * np.log(np.abs(1.0 + c)))[sn]
                fY = np.array(f(Y), dtype=np.float64)
                d = np.where(de, fcur[act] - fY, factor + (fcur[act] - fY))
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
                    walkers=W, stretch=a, kinds=kinds)
    if given:
        res["moves"], res["burn"], res["thin"] = entries, burn, thin
    if reject:
        res["nreject"] = R * (maxiter - 1) - int(nfeas.sum())
    if return_all:
        res["xall"], res["funall"] = squeeze(xall[:, recorded]), squeeze(funall[:, recorded])
    return res
