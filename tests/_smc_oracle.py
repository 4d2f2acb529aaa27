"""numpy restatement of the tempered sequential Monte Carlo sampler (method="smc"; include/stochopy_hip.h states the rule), on
tests/_sample_oracle.py's PhiloxDraws.  Test infrastructure for tests/test_sample_smc_host.py / test_gpu_sample_smc.py.

All populations advance together as (C, P) arrays; every sum over a population is formed in the order the header fixes:

* sum w, sum w^2: thread t of 1 024 owns particles [t K, t K + K), K = ceil(P / 1024), and adds them in index order from 0.0;
  the 64 threads of a wave v += v[lane ^ 1], ^ 2, ... ^ 32; then 0.0 + the 16 waves' sums in order.
* cum: the threads' totals scanned over the wave (v[lane] += v[lane - off], off = 1, 2, ... 32), base = 0.0 + the totals of the
  waves before, then (base + the thread's exclusive value) + its own weights one by one.
* the moments of an axis: 16 partial sums over particles r, r + 16, ..., added in the order of r; two passes.

A missing particle contributes +0.0, which changes no sum of weights, counts or squares.

``nudge``: a function that moves an array's elements at random by one unit in the last place, applied to every weight and every
running sum (the objective's values are the caller's to move): what tests/_smc_cases.admitted uses.
"""
import numpy as np

from _sample_oracle import PURPOSE_PROPOSAL, PhiloxDraws, Result, _in_box, _log_accept
from oracle import objectives
from oracle.streams import philox4x32_10, u53

PURPOSE_RESAMPLE = 18
THREADS, WAVE, HALVINGS = 1024, 64, 52
GATHER_ROWS = 16
MAX_PARTICLES = 16384
RUNNING = 1


def _threads(V):
    """(C, P) -> (C, 1024, K): thread t's particles, missing ones +0.0."""
    C, P = V.shape
    K = -(-P // THREADS)
    out = np.zeros((C, THREADS * K))
    out[:, :P] = V
    return out.reshape(C, THREADS, K)


def _thread_sums(T):
    acc = np.zeros(T.shape[:2])
    for k in range(T.shape[2]):
        acc = acc + T[:, :, k]
    return acc


def pop_sum(V):
    """The sum of each row of V (C, P) in the stage kernel's order."""
    v = _thread_sums(_threads(V)).reshape(V.shape[0], THREADS // WAVE, WAVE)
    lane = np.arange(WAVE)
    off = 1
    while off < WAVE:
        v = v + v[:, :, lane ^ off]
        off *= 2
    acc = np.zeros(V.shape[0])
    for w in range(THREADS // WAVE):
        acc = acc + v[:, w, 0]
    return acc


def pop_cum(W):
    """The inclusive running sums of each row of W (C, P) in the stage kernel's order."""
    C, P = W.shape
    T = _threads(W)
    inc = _thread_sums(T).reshape(C, THREADS // WAVE, WAVE)
    off = 1
    while off < WAVE:
        nxt = inc.copy()
        nxt[:, :, off:] = inc[:, :, off:] + inc[:, :, :-off]
        inc = nxt
        off *= 2
    exc = np.concatenate([np.zeros((C, THREADS // WAVE, 1)), inc[:, :, :-1]], axis=2)
    base = np.zeros((C, THREADS // WAVE))
    acc = np.zeros(C)
    for w in range(THREADS // WAVE):
        base[:, w] = acc
        acc = acc + inc[:, w, WAVE - 1]
    run = (base[:, :, None] + exc).reshape(C, THREADS)
    out = np.empty_like(T)
    for k in range(T.shape[2]):
        run = run + T[:, :, k]
        out[:, :, k] = run
    return out.reshape(C, -1)[:, :P]


def axis_sum(V):
    """The sum over the particles of V (C, P, n) in the gather kernel's order."""
    C, P, n = V.shape
    nb = -(-P // GATHER_ROWS)
    padded = np.zeros((C, nb * GATHER_ROWS, n))
    padded[:, :P] = V
    padded = padded.reshape(C, nb, GATHER_ROWS, n)
    part = np.zeros((C, GATHER_ROWS, n))
    for b in range(nb):
        part = part + padded[:, b]
    acc = np.zeros((C, n))
    for r in range(GATHER_ROWS):
        acc = acc + part[:, r]
    return acc


def axis_sd(X):
    P = X.shape[1]
    mean = axis_sum(X) / P
    d = X - mean[:, None, :]
    return np.sqrt(axis_sum(d * d) / P)


def weights(f, db, fmin, nudge=None):
    """w (C, P) at beta_prev + db (C,): 0 where f is NaN or +inf."""
    ok = np.isfinite(f) | (f == -np.inf)
    with np.errstate(all="ignore"):
        w = np.where(ok, np.exp(-(db[:, None] * (f - fmin[:, None]))), 0.0)
    return w if nudge is None else np.where(ok, nudge(w), 0.0)


def ancestors(cum, u):
    """The least j with cum_j >= ((i + u) / P) cum_{P-1} by the header's bisection; (C, P) int."""
    C, P = cum.shape
    target = ((np.arange(P)[None, :] + u[:, None]) / P) * cum[:, -1:]
    lo = np.zeros((C, P), dtype=np.int64)
    hi = np.full((C, P), P - 1, dtype=np.int64)
    rows = np.arange(C)[:, None]
    while np.any(lo < hi):
        go = lo < hi
        mid = (lo + hi) >> 1
        ge = cum[rows, mid] >= target
        hi = np.where(go & ge, mid, hi)
        lo = np.where(go & ~ge, mid + 1, lo)
    return lo


def sample(fun, bounds, options=None, callback=None, nudge=None, record=False):
    """``fun``: an objective's name or a function (R, n) -> (R,).  Options as stochopy_amd.sample.smc.  ``record``: the result
    also holds, per stage, ``ancs`` (C, P), ``naccs`` (C, P), ``steps_`` (C, n) and ``took`` (C,) (lists over the stages)."""
    o = dict(options or {})
    o.pop("backend", None), o.pop("rng", None)
    C, P, M = o.pop("chains", 1), o.pop("particles", 1024), o.pop("steps", 8)
    maxiter, seed = o.pop("maxiter", 100), o.pop("seed")
    ess, target = o.pop("ess", 0.5), o.pop("target_accept", 0.234)
    pop0 = o.pop("pop0", 0)  # the first population's index among those of a larger call (the keying by global row)
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    scale0 = o.pop("scale", None)
    scale0 = 2.38 / np.sqrt(n) if scale0 is None else float(scale0)
    assert not o, f"unknown options {sorted(o)}"
    f_ = objectives.OBJECTIVES[fun] if isinstance(fun, str) else fun
    R = C * P
    draws = PhiloxDraws(seed, R, n)
    draws.rows = draws.rows + np.uint64(pop0 * P)
    half = 0.5 * (upper - lower)
    pop = np.repeat(np.arange(C), P)

    x = draws.initial(lower, upper)
    with np.errstate(all="ignore"):
        f = np.asarray(f_(x), dtype=np.float64)
    status = np.full(C, RUNNING, dtype=np.int64)
    stages = np.zeros(C, dtype=np.int64)
    beta, logz, scale = np.zeros(C), np.zeros(C), np.full(C, scale0)
    betas, esss, scales, ratios, counts = [beta.copy()], [], [], [], []
    log = {"ancs": [], "naccs": [], "steps_": [], "took": []}
    s = 0
    while np.any(status == RUNNING) and s < maxiter:
        s += 1
        run = status == RUNNING
        F = f.reshape(C, P)
        finite = np.isfinite(F)
        dead = run & (~finite.any(axis=1) | (F == -np.inf).any(axis=1))
        status[dead], logz[dead] = -2, -np.inf
        run = run & ~dead
        if not run.any():
            s -= 1
            break
        fmin = np.where(finite, F, np.inf).min(axis=1)
        fmin = np.where(run, fmin, 0.0)
        thr = ess * float(P)

        def ess_of(b):
            w = weights(F, b - beta, fmin, nudge)
            sw, sw2 = pop_sum(w), pop_sum(w * w)
            with np.errstate(all="ignore"):
                return sw, sw2, (sw * sw) / sw2 >= thr

        _, _, one = ess_of(np.ones(C))
        lo, hi = beta.copy(), np.ones(C)
        for _ in range(HALVINGS):
            mid = (lo + hi) / 2.0
            _, _, ok = ess_of(mid)
            lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
        new = np.where(one, 1.0, np.where(lo > beta, lo, hi))
        new = np.where(run, new, beta)
        db = new - beta
        sw, sw2, _ = ess_of(new)
        with np.errstate(all="ignore"):
            logz = np.where(run, logz + (np.log(sw / float(P)) - db * fmin), logz)
            esss.append(np.where(run, ((sw * sw) / sw2) / float(P), 0.0))
        beta = new
        # step 3
        w = weights(F, db, fmin, nudge)
        cum = pop_cum(w)
        if nudge is not None:
            cum = nudge(cum)
        words = philox4x32_10(np.zeros((1, 1), dtype=np.uint64), ((np.arange(C) + pop0) * P).astype(np.uint64)[:, None], s,
                              PURPOSE_RESAMPLE, draws.k0, draws.k1)
        u = u53(words[0], words[1])[:, 0]
        anc = ancestors(cum, u)
        anc = np.where(run[:, None], anc, np.arange(P)[None, :])
        src = (anc + np.arange(C)[:, None] * P).reshape(R)
        x, f = x[src], f[src]
        # step 4
        sd = axis_sd(x.reshape(C, P, n))
        floor = 1.0e-8 * half
        step = scale[:, None] * np.where(sd > floor, sd, floor)
        scales.append(np.where(run, scale, 0.0))
        # step 5
        live = run[pop]
        nacc = np.zeros(R, dtype=np.int64)
        for m in range(1, M + 1):
            g = (s - 1) * M + m
            prop = x + draws.normals(0, n, g, PURPOSE_PROPOSAL) * step[pop]
            with np.errstate(all="ignore"):
                fprop = np.asarray(f_(prop), dtype=np.float64)
                d = beta[pop] * (f - fprop)
            accept = live & _in_box(prop, lower, upper) & _log_accept(d, draws.accept_uniform(g, None))
            nacc += accept
            x = np.where(accept[:, None], prop, x)
            f = np.where(accept, fprop, f)
        # step 6
        count = nacc.reshape(C, P).sum(axis=1)
        r = count / (float(P) * float(M))
        ratios.append(np.where(run, r, 0.0))
        counts.append(np.where(run, count, 0))
        scale = np.where(run, scale * np.exp(r - target), scale)
        stages[run] = s
        status[run & (beta == 1.0)] = 0
        if s >= maxiter:
            status[status == RUNNING] = -1
        betas.append(beta.copy())
        if record:
            log["ancs"].append(anc), log["naccs"].append(nacc.reshape(C, P)), log["steps_"].append(step), log["took"].append(run)
        if callback is not None:
            callback(_squeeze(x.reshape(C, P, n), C), Result(nit=s, betas=_squeeze(np.array(betas).T, C), log_evidence=_squeeze(logz.copy(), C)))
    S = s
    b = int(np.argmin(f))
    attempted = P * M * int(stages.sum())
    res = Result(x=x[b], fun=f[b], nit=S, status=int(status.min()), particles=P,
                 accept_ratio=float(np.sum(counts)) / attempted if attempted else 0.0,
                 nfev=int(np.sum(P * (1 + M * stages))))
    for name, value in (("xall", x.reshape(C, P, n)), ("funall", f.reshape(C, P)), ("log_evidence", logz),
                        ("betas", np.array(betas).T), ("stages", stages), ("statuses", status),
                        ("accept_ratios", np.array(ratios).reshape(S, C).T), ("scales", np.array(scales).reshape(S, C).T),
                        ("ess", np.array(esss).reshape(S, C).T)):
        res[name] = _squeeze(np.ascontiguousarray(value), C)
    if record:
        res.update(log)
        res["counts"] = np.array(counts).reshape(S, C).T
    return res


def _squeeze(v, C):
    return v[0] if C == 1 else v
