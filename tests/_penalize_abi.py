"""constraints="Penalize" on the device, one call at a time (sx_cma_penalize: cma_rank_kernel -> cma_penalty_kernel ->
sx_cmaes_eval_penalized -> cma_add_penalty_kernel, csrc/sx_cma_loop.hip): the planted states that
tests/test_gpu_penalize.py runs and tests/test_penalize_host.py checks on the CPU, the restatement of
oracle.engine.PenalizeState.apply in a number format of the caller's choice, and the packing of the workspace
`w[n] | v[n] | pen[P] | hist[256] | count, valid, ini, -`.  A plain helper module (imported, not collected); nothing here
touches the device at import.

The launch ranks and takes percentiles of the `fit` it is GIVEN and only afterwards replaces it by the objective of the
clipped `arx` plus the penalty, so a case plants its percentile inputs freely; the oracle is driven the same way (its `fun`
hands back the planted values)."""
import collections
import functools
import os
import re
import zlib

import numpy as np

from oracle import engine

LD = np.longdouble
U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTIVES = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")


def _constant(name):
    with open(os.path.join(ROOT, "stochopy_amd", "csrc", "sx_cma_loop.hip")) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


PATH_THREADS = _constant("kPathThreads")  # the element loops of cma_penalty_kernel stride by this
HIST = _constant("kPenHist")              # slots of the spread history
SENTINEL = 7.0                            # what the unused history slots of a case hold (+ k 2^-20)


def cap(n, P):
    return 20.0 + (3.0 * n) / P


def admitted(n, P):
    """The guard of cma_penalize_launch (and optimize/_evolution.py device_loop_serves)."""
    return cap(n, P) + 1.0 <= HIST


# ---- workspace -----------------------------------------------------------------------------------------------------------
def pack_ws(n, P, w, hist, count, valid, ini):
    """hist: the `count` live entries; the other slots get distinct sentinels, v and pen a NaN that must be overwritten."""
    ws = np.empty(2 * n + P + HIST + 4)
    ws[:n] = w
    ws[n:2 * n + P] = np.nan
    ws[2 * n + P:2 * n + P + HIST] = SENTINEL + np.arange(HIST) * 2.0 ** -20
    ws[2 * n + P:2 * n + P + len(hist)] = hist
    ws[2 * n + P + HIST:] = (count, valid, ini, -3.0)
    return ws


def unpack_ws(ws, n, P):
    h = 2 * n + P
    return dict(w=ws[:n].copy(), v=ws[n:2 * n].copy(), pen=ws[2 * n:h].copy(), hist=ws[h:h + HIST].copy(),
                count=ws[h + HIST], valid=ws[h + HIST + 1], ini=ws[h + HIST + 2], spare=ws[h + HIST + 3])


# ---- cases ---------------------------------------------------------------------------------------------------------------
# form: "cma" (the diagonal of a planted C) or "vd" (d (1 + v^2) d of planted dvec, vvec); diag: cma -- the diagonal; vd -- None
Case = collections.namedtuple("Case", "tag form n P gen fun fit w hist count valid ini xmean xold sigma mueff diag dvec vvec "
                                      "arx xm xstd")


def mueff_of(P):
    mu = max(1, int(0.5 * P))
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    w /= w.sum()
    return float(w.sum() ** 2 / np.square(w).sum())


def _rs(tag):
    return np.random.RandomState(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


def make(tag, form, n, P, gen=3, count=5, valid=1, ini=0, outside=(), fit=None, hist=None, diag=None, sigma=0.3, w=None,
         xmean=None, xold=None):
    """A planted state.  Defaults: distinct fitness values, weights in [0.5, 2], `count` history entries in [0.1, 10], a mean
    inside the box, a diagonal in [0.5, 2]; `outside`: coordinates of the mean put at 1.6 + 0.6 e / n, moving outwards."""
    rs = _rs(tag)
    fit = rs.permutation(P) * 1.25 + rs.uniform(1.0, 2.0, P) if fit is None else np.asarray(fit, dtype=np.float64)
    w = rs.uniform(0.5, 2.0, n) if w is None else np.asarray(w, dtype=np.float64)
    hist = rs.uniform(0.1, 10.0, count) if hist is None else np.asarray(hist, dtype=np.float64)
    assert len(hist) == count and len(fit) == P
    xm0 = rs.uniform(-0.9, 0.9, n)
    for e in outside:
        xm0[e] = 1.6 + 0.6 * e / n
    xmean = xm0 if xmean is None else np.asarray(xmean, dtype=np.float64)
    xold = xmean - rs.uniform(0.01, 0.1, n) * np.where(xmean < 0.0, -1.0, 1.0) if xold is None else np.asarray(xold, dtype=np.float64)
    target = rs.uniform(0.5, 2.0, n) if diag is None else np.asarray(diag, dtype=np.float64)
    dvec = vvec = None
    if form == "vd":
        vvec = rs.uniform(-1.0, 1.0, n)
        dvec = np.sqrt(target / (1.0 + vvec * vvec))
        target = None
    arx = rs.uniform(-1.5, 1.5, (P, n))
    fun = OBJECTIVES[zlib.crc32(tag.encode()) % len(OBJECTIVES)]
    xm, xstd = rs.uniform(-1.0, 1.0, n), rs.uniform(0.5, 2.0, n)
    return Case(tag, form, n, P, gen, fun, fit, w, hist, count, valid, ini, xmean, xold, sigma, mueff_of(P), target, dvec,
                vvec, arx, xm, xstd)


def diagonal(case, T=np.float64):
    if case.form == "vd":
        d, v = case.dvec.astype(T), case.vvec.astype(T)
        return (d * (1 + v * v)) * d
    return case.diag.astype(T)


def c_matrix(case):
    """A full (n, n) C around the planted diagonal: the kernel must read the diagonal only."""
    C = _rs(case.tag + "C").uniform(-5.0, 5.0, (case.n, case.n))
    C[np.arange(case.n), np.arange(case.n)] = case.diag
    return C


NS = (1, 2, 63, 64, 65, PATH_THREADS - 1, PATH_THREADS, PATH_THREADS + 1)
PS = (2, 3, 4, 5, 8, 70)
FORMS = ("cma", "vd")


def _threshold(case, T=LD):
    """kk sqrt(dc): what |tx| is compared with (cmaes/_constraints.py:64-66)."""
    n = case.n
    return 3 * max(T(1), np.sqrt(T(n) / T(case.mueff))) * T(case.sigma) * np.sqrt(diagonal(case, T))


def _growth_case(form):
    """Eight coordinates; each of the three conditions of the growth (outside, |tx| > kk sqrt(dc), sign(tx) == sign(xmean -
    xold)) fails alone somewhere, and the threshold is approached from both sides at a relative distance of 1e-6."""
    n, P = 8, 6
    base = make("growth-" + form, form, n, P, ini=0)
    thr = _threshold(base).astype(np.float64)
    xmean = np.array([0.3,                       # 0 inside: never grows
                      1.0 + 4.0 * thr[1],        # 1 outside, far, moving outwards: grows
                      1.0 + thr[2] * (1 - 1e-6),  # 2 outside, just short of the threshold, moving outwards: does not
                      1.0 + 4.0 * thr[3],        # 3 outside, far, moving INWARDS: does not
                      1.0 + 4.0 * thr[4],        # 4 outside, far, xmean == xold: sign 0 != 1: does not
                      -1.0 - 4.0 * thr[5],       # 5 below -1, xmean == xold: tx = 0 (only the upper side is clipped), 0 == 0 but |0| > thr fails
                      1.0 + thr[6] * (1 + 1e-6),  # 6 outside, just past the threshold, moving outwards: grows
                      -1.0 - 4.0 * thr[7]])      # 7 below -1, moving outwards: tx = 0: does not
    step = np.array([0.05, 0.05, 0.05, -0.05, 0.0, 0.0, 0.05, -0.05])
    return base._replace(xmean=xmean, xold=xmean - step)


@functools.lru_cache(maxsize=None)
def cases():
    """tag -> Case, every planted state of the bookkeeping tests."""
    out = []
    for form in FORMS:
        # every shape the guard admits: first call after the warm-up with the mean outside -- percentiles, push, median,
        # fill, growth and v in one call (every third coordinate and the last).  The step size puts the growth
        # threshold 0.9 sqrt(dc) among the excesses 0.6 ... 1.2: some of the outside coordinates grow, some do not.
        for n in NS:
            for P in PS:
                if admitted(n, P):
                    out.append(make("shape-%s-n%d-P%d" % (form, n, P), form, n, P, gen=3, count=7, valid=1, ini=1,
                                    outside=tuple(sorted(set(range(0, n, 3)) | {n - 1})), sigma=0.3 / max(1.0, np.sqrt(n / mueff_of(P)))))
        # first generation: history [1.0], valid 0, ini 1
        out.append(make("first-inside-" + form, form, 4, 6, gen=1, count=1, hist=[1.0], valid=0, ini=1, w=np.zeros(4)))
        out.append(make("first-outside-" + form, form, 4, 6, gen=1, count=1, hist=[1.0], valid=0, ini=1, w=np.zeros(4),
                        outside=(2,)))
        # delta == 0 in the first generation: everything equal; only the middle half tied (P = 8: ranks 1 .. 6)
        out.append(make("flat-all-" + form, form, 4, 8, gen=1, count=1, hist=[1.0], valid=0, ini=1, fit=np.full(8, 3.5)))
        out.append(make("flat-middle-" + form, form, 4, 8, gen=1, count=1, hist=[1.0], valid=0, ini=1,
                        fit=[2.0, 9.0, 2.0, -1.0, 2.0, 2.0, 2.0, 2.0]))
        # delta == 0 with zeros, a NaN and positives in the history: the smallest POSITIVE entry
        out.append(make("flat-mixed-" + form, form, 4, 8, gen=5, count=7, hist=[0.0, np.nan, 3.0, 0.5, -0.0, 2.0, 0.0], valid=1,
                        ini=1, fit=np.full(8, -2.25)))
        # the sliding window: an integral cap (n = 4, P = 6: 22, strict <) and a fractional one (n = 6, P = 12: 21.5)
        for n, P in ((4, 6), (6, 12)):
            for count in (20, 21, 22, 23):
                out.append(make("window-%s-n%d-c%d" % (form, n, count), form, n, P, gen=30, count=count, valid=1, ini=1,
                                outside=(1,)))
        # the largest history the guard admits (n = 470, P = 6: cap 255): pushes to 254 and 255 entries, shifts at 255; the
        # median of an even and an odd number of unsorted entries with duplicates and a descending run
        for count in (253, 254, 255):
            rs = _rs("largest%d" % count)
            hist = rs.uniform(0.1, 10.0, count)
            hist[10:60] = np.linspace(9.0, 1.0, 50)   # descending run
            hist[100:140] = hist[30:70]                # duplicates
            hist[200:220] = 4.25
            out.append(make("largest-%s-c%d" % (form, count), form, 470, 6, gen=400, count=count, hist=hist, valid=1, ini=1,
                            outside=(0, 469)))
        # the phase flags: ini x valid x gen x (mean inside / one coordinate outside); with valid 0 both a generation that
        # sets it (delta != 0) and a flat one that does not
        for ini in (0, 1):
            for valid in (0, 1):
                for gen in (1, 2, 3):
                    for out_ in (0, 1):
                        for flat in ((0, 1) if valid == 0 else (0,)):
                            tag = "phase-%s-i%d-v%d-g%d-o%d-f%d" % (form, ini, valid, gen, out_, flat)
                            out.append(make(tag, form, 5, 6, gen=gen, count=4, valid=valid, ini=ini,
                                            outside=(3,) if out_ else (), fit=np.full(6, 1.5) if flat else None))
        out.append(_growth_case(form))
        # a diagonal spanning 1e-8 ... 1: the scale exp(0.9 (log dc - mean log dc)) of v
        diag = np.logspace(-8.0, 0.0, 64)[_rs("span").permutation(64)]
        out.append(make("span-" + form, form, 64, 8, gen=3, count=6, valid=1, ini=1, diag=diag, outside=(0, 5, 63), sigma=1e-3))
    assert len({c.tag for c in out}) == len(out)
    return collections.OrderedDict((c.tag, c) for c in out)


def tags():
    return list(cases())


# ---- the restatement -----------------------------------------------------------------------------------------------------
Outcome = collections.namedtuple("Outcome", "delta fresh hist count valid ini filled fill grown w v fac outside margin")


def restate(case, T=LD):
    """oracle.engine.PenalizeState.apply (cmaes/_constraints.py:33-76) on the planted state, in the number format T.  The
    quartiles are np.percentile's of the planted (double) fitness; everything after them is carried in T.  `fresh`: the new
    history entry was computed (False: it is a copy of an old entry, delta == 0); `margin`: over the coordinates outside
    the box, the smallest relative distance of |tx| from the threshold it is compared with."""
    n, P = case.n, case.P
    q25, q75 = np.percentile(case.fit, [25.0, 75.0])
    diag = diagonal(case, T)
    sigma, mueff = T(case.sigma), T(case.mueff)
    with np.errstate(invalid="ignore"):
        spread = T(q75) - T(q25) if T is not np.float64 else q75 - q25
        delta = spread / n / (diag.sum() / n) / (sigma * sigma)
        hist = [T(h) for h in case.hist[:case.count]]
        valid, ini, fresh = int(case.valid), int(case.ini), True
        if delta == 0:
            pos = [h for h in hist if h > 0]
            delta, fresh = (min(pos) if pos else T(np.inf)), False
        elif not valid:
            hist, valid = [], 1
    hist = hist + [delta] if len(hist) < cap(n, P) else hist[1:] + [delta]
    xmean, xold = case.xmean.astype(T), case.xold.astype(T)
    outside = (xmean < -1) | (xmean > 1)
    w, filled, fill = case.w.astype(T), False, None
    if ini and outside.any():
        s = sorted(hist)
        m = len(s)
        fill = T(2.0002) * (s[m // 2] if m & 1 else (s[m // 2 - 1] + s[m // 2]) / 2)
        w, filled = np.full(n, fill, dtype=T), True
        if valid and case.gen > 2:
            ini = 0
    grown, margin = np.zeros(n, dtype=bool), np.inf
    fac = T(1.2) ** min(T(1), mueff / 10 / n)
    if outside.any():
        tx = xmean - np.where(xmean > 1, T(1), xmean)
        thr = _threshold(case, T)
        grown = outside & (np.abs(tx) > thr) & (np.sign(tx) == np.sign(xmean - xold))
        margin = float(np.min(np.abs(np.abs(tx[outside]) - thr[outside]) / thr[outside]))
        w = np.where(grown, w * fac, w)
    logd = np.log(diag)
    v = w / np.exp(T(0.9) * (logd - logd.sum() / n))
    return Outcome(delta, fresh, hist, len(hist), valid, ini, filled, fill, grown, w, v, fac, outside, margin)


def oracle_apply(case):
    """oracle.engine.PenalizeState itself from the planted state: (state after, fitness returned, clipped candidates)."""
    st = engine.PenalizeState(case.n)
    st.weights = case.w.copy()
    st.dfithist = np.array(case.hist[:case.count], dtype=np.float64)
    st.validfitval, st.iniphase = bool(case.valid), bool(case.ini)
    with np.errstate(invalid="ignore"):
        fit, clipped = st.apply(case.arx, case.xmean, case.xold, case.sigma, diagonal(case), case.mueff, case.gen,
                                lambda X: case.fit.copy())
    return st, fit, clipped


def kernel_quartiles(fit):
    """cma_penalty_kernel's q25, q75 stated in numpy: the virtual index (P - 1) q, the two neighbours in the stable order,
    numpy's _lerp."""
    fit = np.asarray(fit, dtype=np.float64)
    P = len(fit)
    order = np.argsort(fit, kind="stable")
    out = []
    for q in (0.25, 0.75):
        vi = np.float64(P - 1) * q
        lo = int(np.floor(vi))
        hi = lo + 1 if lo + 1 < P else P - 1
        a, b, t = fit[order[lo]], fit[order[hi]], vi - np.float64(lo)
        d = b - a
        out.append(b - d * (1.0 - t) if t >= 0.5 else a + d * t)
    return np.array(out)


# ---- the device ----------------------------------------------------------------------------------------------------------
def state_word(sigma, done=0):
    from stochopy_amd import _lib

    st = _lib.SxCmaState(it=0, nfev=0, best_row=-1, fbest=0.0, sigma=sigma, sigma_next=sigma, tmp_coef=0.0, psnorm=0.0,
                         status=_lib.SX_STATUS_NONE, done=done, stop_it=0)
    return np.frombuffer(bytes(st), dtype=np.float64).copy()


Device = collections.namedtuple("Device", "rc message ws ws_before fit order f_raw state state_before")


def run(ctx, case, done=0):
    """Plant the case, call sx_cma_penalize once, read everything back; f_raw: sx_cmaes_eval_penalized's objective of the
    clipped candidates on its own (what the launch adds the penalty to)."""
    import ctypes as C

    from stochopy_amd import _device, _lib

    t, p = _device.torch(), _device.ptr
    n, P = case.n, case.P
    ws0 = pack_ws(n, P, case.w, case.hist, case.count, case.valid, case.ini)
    st0 = state_word(case.sigma, done)
    keep = dict(arx=ctx.upload(case.arx), fit=ctx.upload(case.fit), xm=ctx.upload(case.xm), xstd=ctx.upload(case.xstd),
                xmean=ctx.upload(case.xmean), xold=ctx.upload(case.xold), state=ctx.upload(st0), pen_ws=ctx.upload(ws0),
                pen_order=ctx.upload(np.full(P, -1, dtype=np.int64)))
    dvec = vvec = None
    if case.form == "vd":
        dvec, vvec = ctx.upload(case.dvec), ctx.upload(case.vvec)
    else:
        keep["C"] = ctx.upload(c_matrix(case))
    a = _lib.SxCmaArgs(**{k: p(v) for k, v in keep.items()})
    a.n, a.P, a.mueff, a.fun_id = n, P, case.mueff, _lib.FUN_IDS[case.fun]
    f_raw = ctx.empty((P,))
    with t.cuda.stream(ctx.stream):
        rc = ctx.L.sx_cma_penalize(C.byref(a), case.gen, p(dvec) if dvec is not None else None,
                                   p(vvec) if vvec is not None else None, ctx.stream_ptr)
        message = ctx.L.sx_last_error().decode() if rc else ""
        _lib.check(ctx.L.sx_cmaes_eval_penalized(a.fun_id, p(keep["arx"]), P, n, p(keep["xm"]), p(keep["xstd"]), None, p(f_raw),
                                                 None, ctx.stream_ptr), "sx_cmaes_eval_penalized")
    ctx.sync()
    rd = lambda x: x.cpu().numpy()  # noqa: E731
    return Device(rc, message, rd(keep["pen_ws"]), ws0, rd(keep["fit"]), rd(keep["pen_order"]), rd(f_raw), rd(keep["state"]),
                  st0)
