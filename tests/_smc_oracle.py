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

``sample`` is built from ``stage_once``, ``gather_once`` and ``mutate_once``, one entry point of the library each, on explicit
state: what tests/test_gpu_sample_smc_kernels.py holds a single kernel call against (tests/_smc_kernel_cases.py).
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


# ---- one step at a time: what tests/test_gpu_sample_smc_kernels.py holds one kernel call against ------------------------------
ST_STATUS, ST_BETA, ST_LOGZ, ST_ESS, ST_SCALE, ST_ACCEPT, ST_STAGES, ST_COUNT, ST_WORDS = range(9)


def start_records(C, scale):
    record = np.zeros((C, ST_WORDS))
    record[:, ST_STATUS], record[:, ST_SCALE] = RUNNING, scale
    return record


def stage_once(F, record, s, P, ess, target, M, maxiter, key, nacc, pop0=0, nudge=None):
    """sx_smc_stage(s) on the records (C, 8): step 6 of stage s - 1 for the populations whose [6] is s - 1 (``nacc`` (C, P), the
    counts of its mutation), then steps 1 - 3 of stage s on the values ``F`` (C, P) for those still running.  ``key`` = (key0,
    key1).  Returns the new records and the ancestors (C, P); a population that takes no part (its new [6] is not s) has the
    identity there -- the kernel leaves its anc alone."""
    F = np.asarray(F, dtype=np.float64).reshape(-1, P)
    C = F.shape[0]
    rec = np.array(record, dtype=np.float64).reshape(C, ST_WORDS)
    beta, logz, scale = rec[:, ST_BETA].copy(), rec[:, ST_LOGZ].copy(), rec[:, ST_SCALE].copy()
    if s >= 2:  # step 6
        six = rec[:, ST_STAGES] == float(s - 1)
        count = np.asarray(nacc).reshape(C, P).sum(axis=1)
        r = count / (float(P) * float(M))
        scale = np.where(six, scale * np.exp(r - target), scale)
        rec[:, ST_ACCEPT] = np.where(six, r, rec[:, ST_ACCEPT])
        rec[:, ST_COUNT] = np.where(six, count, rec[:, ST_COUNT])
    run = rec[:, ST_STATUS] == RUNNING
    finite = np.isfinite(F)
    dead = run & (~finite.any(axis=1) | (F == -np.inf).any(axis=1))
    rec[dead, ST_STATUS], rec[dead, ST_LOGZ] = -2, -np.inf
    run = run & ~dead
    anc = np.tile(np.arange(P), (C, 1))
    if not run.any():
        return rec, anc
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
        ess_new = ((sw * sw) / sw2) / float(P)
    # step 3
    w = weights(F, db, fmin, nudge)
    cum = pop_cum(w)
    if nudge is not None:
        cum = nudge(cum)
    k0, k1 = key
    words = philox4x32_10(np.zeros((1, 1), dtype=np.uint64), ((np.arange(C) + pop0) * P).astype(np.uint64)[:, None], s,
                          PURPOSE_RESAMPLE, k0, k1)
    u = u53(words[0], words[1])[:, 0]
    anc = np.where(run[:, None], ancestors(cum, u), anc)
    status = np.where(new == 1.0, 0.0, -1.0 if s >= maxiter else float(RUNNING))
    for word, value in ((ST_STATUS, status), (ST_BETA, new), (ST_LOGZ, logz), (ST_ESS, ess_new), (ST_SCALE, scale),
                        (ST_STAGES, float(s))):
        rec[:, word] = np.where(run, value, rec[:, word])
    return rec, anc


def gather_once(x, f, anc, scale, lower, upper):
    """sx_smc_resample on populations that take part: x (C, P, n), f (C, P) through anc (C, P; held inside [0, P) whatever it
    holds) and step 4 with scale (C,).  Returns the moved x and f and the steps (C, n)."""
    C, P, n = x.shape
    anc = np.clip(np.asarray(anc, dtype=np.int64), 0, P - 1)
    rows = np.arange(C)[:, None]
    x, f = x[rows, anc], f[rows, anc]
    sd = axis_sd(x)
    floor = 1.0e-8 * (0.5 * (np.asarray(upper, dtype=np.float64) - np.asarray(lower, dtype=np.float64)))
    step = np.asarray(scale, dtype=np.float64)[:, None] * np.where(sd > floor, sd, floor)
    return x, f, step


def mutate_once(x, f, step, beta, live, s, M, key, lower, upper, fun, pop0=0, trace=None):
    """sx_smc_mutate(s): the M Metropolis steps of step 5 on x (C, P, n), f (C, P) with step (C, n) and beta (C,); the
    populations that are not ``live`` (C,) propose along and keep what they hold.  ``fun``: (C P, n) -> (C P,).  Returns the
    new x and f and the accepted steps (C, P).  ``trace``: a list that receives, per step, (outside the box, accepted) (C P,)."""
    C, P, n = x.shape
    R = C * P
    draws = PhiloxDraws(int(key[0]) | (int(key[1]) << 32), R, n)
    draws.rows = draws.rows + np.uint64(pop0 * P)
    pop = np.repeat(np.arange(C), P)
    x, f = x.reshape(R, n), f.reshape(R)
    livep = np.asarray(live, dtype=bool)[pop]
    nacc = np.zeros(R, dtype=np.int64)
    for m in range(1, M + 1):
        g = (s - 1) * M + m
        prop = x + draws.normals(0, n, g, PURPOSE_PROPOSAL) * step[pop]
        with np.errstate(all="ignore"):
            fprop = np.asarray(fun(prop), dtype=np.float64)
            d = beta[pop] * (f - fprop)
        inside = _in_box(prop, lower, upper)
        accept = livep & inside & _log_accept(d, draws.accept_uniform(g, None))
        if trace is not None:
            trace.append((~inside, accept))
        nacc += accept
        x = np.where(accept[:, None], prop, x)
        f = np.where(accept, fprop, f)
    return x.reshape(C, P, n), f.reshape(C, P), nacc.reshape(C, P)


def sample(fun, bounds, options=None, callback=None, nudge=None, record=False):
    """``fun``: an objective's name or a function (R, n) -> (R,).  Options as stochopy_amd.sample.smc.  ``record``: the result
    also holds, per stage, ``ancs`` (C, P), ``naccs`` (C, P), ``steps_`` (C, n) and ``took`` (C,) (lists over the stages), and the
    particles after stage 0, ``x0`` (C, P, n) / ``f0`` (C, P).  The run is stage_once, gather_once and mutate_once in the order
    stochopy_amd.sample._smc.run calls their entry points."""
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
    key = (draws.k0, draws.k1)

    x = draws.initial(lower, upper).reshape(C, P, n)
    with np.errstate(all="ignore"):
        f = np.asarray(f_(x.reshape(R, n)), dtype=np.float64).reshape(C, P)
    rec = start_records(C, scale0)
    nacc = np.zeros((C, P), dtype=np.int64)
    stages = np.zeros(C, dtype=np.int64)
    betas, esss, scales, ratios, counts = [rec[:, ST_BETA].copy()], [], [], [], []
    log = {"ancs": [], "naccs": [], "steps_": [], "took": [], "x0": x, "f0": f}

    def step_six(of):  # r and the count of stage ``of``, for the populations that took part in it
        ratios.append(np.where(stages == of, rec[:, ST_ACCEPT], 0.0))
        counts.append(np.where(stages == of, rec[:, ST_COUNT], 0.0).astype(np.int64))

    S, closed = 0, False
    while np.any(rec[:, ST_STATUS] == RUNNING) and S < maxiter:
        S += 1
        rec, anc = stage_once(f, rec, S, P, ess, target, M, maxiter, key, nacc, pop0, nudge)
        if S >= 2:
            step_six(S - 1)
        took = rec[:, ST_STAGES] == float(S)
        if not took.any():  # (every population still running ended at the start of this stage: status -2)
            S, closed = S - 1, True
            break
        stages = rec[:, ST_STAGES].astype(np.int64)
        x, f, step = gather_once(x, f, anc, rec[:, ST_SCALE], lower, upper)
        x, f, nacc = mutate_once(x, f, step, rec[:, ST_BETA], took, S, M, key, lower, upper, f_, pop0)
        esss.append(np.where(took, rec[:, ST_ESS], 0.0))
        scales.append(np.where(took, rec[:, ST_SCALE], 0.0))
        betas.append(rec[:, ST_BETA].copy())
        if record:
            log["ancs"].append(anc), log["naccs"].append(nacc), log["steps_"].append(step), log["took"].append(took)
        if callback is not None:
            callback(_squeeze(x.copy(), C), Result(nit=S, betas=_squeeze(np.array(betas).T, C), log_evidence=_squeeze(rec[:, ST_LOGZ].copy(), C)))
    if S >= 1 and not closed:  # step 6 of the last stage
        rec, _ = stage_once(f, rec, S + 1, P, ess, target, M, maxiter, key, nacc, pop0, nudge)
        step_six(S)
    status, logz = rec[:, ST_STATUS].astype(np.int64), rec[:, ST_LOGZ].copy()
    x, f = x.reshape(R, n), f.reshape(R)
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
