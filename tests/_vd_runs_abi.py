"""The batched-runs VD-CMA kernel (csrc/sx_vd_runs.hip) through its C ABI, restated for the tests: the LDS layout the kernel's
header comment documents, in bytes; launch_runs, one sx_vd_runs_launch filled as optimize/_vdcma.py _minimize_runs fills it
but with real nfevs / sigmas / xmeans / dvecs / vvecs buffers; and a plain numpy generation 1.  A plain helper module
(imported, not collected)."""

import math

import numpy as np

LDS_LIMIT = 160 * 1024
MIN_DIM = 6


def lanes_per_row(n):
    return 16 if n <= 64 else (32 if n <= 128 else 64)


def threads(n):
    return 256 if n <= 128 else 512


def row_stride(n):
    """gen_row_stride of csrc/sx_device.hpp: the staged vector, 8 doubles of padding, the long rows' leaf sums."""
    return n + 8 if n <= 256 else n + 8 + 2 * (n // 64 + 2)


def npair(n):
    lpr = lanes_per_row(n)
    return -(-n // (2 * lpr)) * lpr


def slices(n):
    return min(8, max(1, threads(n) // npair(n)))


def lds_bytes(P, n):
    """11 vectors of n | fit, t, t_k [P] | order[P] as int32 | red[80] | pos[8] | max(staging rows, pass 2's partial sums)."""
    stage = (threads(n) // lanes_per_row(n)) * row_stride(n)
    part = 8 * slices(n) * npair(n)
    return 8 * (11 * n + 3 * P + (P + 1) // 2 + 88 + max(stage, part))


def workspace_bytes(R, maxiter):
    return 8 * R * maxiter


def largest(fits, lo, hi):
    """The largest k in [lo, hi) with fits(k), fits being true up to some point and false beyond."""
    assert fits(lo) and not fits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if fits(mid):
            lo = mid
        else:
            hi = mid
    return lo


def largest_popsize(lib, n):
    return largest(lambda p: lib.sx_vd_runs_lds_bytes(p, n) > 0, 2, 1 << 20)


def largest_popsize_below(limit_bytes, n):
    return largest(lambda p: lds_bytes(p, n) <= limit_bytes, 2, 1 << 20)


def default_popsize(n):
    return 4 + int(math.floor(3.0 * math.log(n)))


def launch_runs(objective, lower, upper, P, seeds, x0=None, maxiter=100, sigma=0.1, muperc=0.5, xtol=1e-8, ftol=1e-8):
    """One sx_vd_runs_launch of len(seeds) runs of `objective` (a factory name) with every optional output.  lower / upper:
    one value per dimension.  x0: None, (n,) or (R, n), in the caller's coordinates.  Returns a dict of numpy arrays: xs, funs,
    nits, statuses, nfevs, sigmas, xmeans (standardised), dvecs, vvecs."""
    import ctypes as C

    from stochopy_amd import _device, _lib, _rng
    from stochopy_amd.optimize._vdcma import _strategy_constants

    seeds = [int(s) for s in seeds]
    R = len(seeds)
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    n = len(lower)
    mu, w, mueff, cc, c1, cmu = _strategy_constants(n, P, muperc)
    xm, xstd = 0.5 * (upper + lower), 0.5 * (upper - lower)
    xmean0, vvec0 = np.empty((R, n)), np.empty((R, n))
    if x0 is not None:
        xmean0[:] = (np.asarray(x0, dtype=np.float64) - xm) / xstd
    for r, s in enumerate(seeds):
        init = np.random.RandomState(s & 0xFFFFFFFF)
        if x0 is None:
            xmean0[r] = init.uniform(-1.0, 1.0, n)
        vvec0[r] = init.randn(n) / np.sqrt(n)

    ctx = _device.Context()
    t = _device.torch()
    with t.cuda.stream(ctx.stream):
        keys = np.array([_rng.philox_key(s) for s in seeds], dtype=np.uint32)
        d_keys = ctx.upload_async(keys.view(np.int32))
        d_xmean0, d_vvec0, d_w = ctx.upload(xmean0), ctx.upload(vvec0), ctx.upload(w)
        d_std = ctx.upload_async(np.concatenate([xm, xstd]))
        d_work = ctx.empty((int(ctx.L.sx_vd_runs_workspace_bytes(R, maxiter)) // 8,))
        fill = -12345.678  # no run produces it: an element the kernel does not write cannot pass for a result
        xs, xmeans, dvecs, vvecs = [t.full((R, n), fill, dtype=t.float64, device=ctx.device) for _ in range(4)]
        funs, sigmas = [t.full((R,), fill, dtype=t.float64, device=ctx.device) for _ in range(2)]
        nits, nfevs = [t.full((R,), -7, dtype=t.int64, device=ctx.device) for _ in range(2)]
        statuses = t.full((R,), 77, dtype=t.int32, device=ctx.device)
        a = _lib.SxVdRunsArgs()
        a.keys, a.xmean0, a.vvec0, a.w = d_keys.data_ptr(), d_xmean0.data_ptr(), d_vvec0.data_ptr(), d_w.data_ptr()
        a.xm, a.xstd = d_std[:n].data_ptr(), d_std[n:].data_ptr()
        a.work, a.xs, a.funs, a.nits, a.statuses = (d_work.data_ptr(), xs.data_ptr(), funs.data_ptr(), nits.data_ptr(),
                                                    statuses.data_ptr())
        a.nfevs, a.sigmas, a.xmeans, a.dvecs, a.vvecs = (nfevs.data_ptr(), sigmas.data_ptr(), xmeans.data_ptr(),
                                                         dvecs.data_ptr(), vvecs.data_ptr())
        a.R, a.P, a.n, a.mu, a.fun_id, a.maxiter = R, P, n, mu, _lib.FUN_IDS[objective], maxiter
        a.ilim = int(10.0 + 30.0 * n / P)
        a.mueff, a.cc, a.c1, a.cmu = mueff, cc, c1, cmu
        a.cs, a.ds, a.wsum = 0.3, float(np.sqrt(n)), float(w.sum())
        a.sigma = a.insigma = sigma
        a.xtol, a.ftol = xtol, ftol
        _lib.check(ctx.L.sx_vd_runs_launch(C.byref(a), ctx.stream_ptr), "sx_vd_runs_launch")
        out = dict(xs=xs, funs=funs, nits=nits, statuses=statuses, nfevs=nfevs, sigmas=sigmas, xmeans=xmeans, dvecs=dvecs,
                   vvecs=vvecs)
        out = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("xs", "xmeans", "dvecs", "vvecs", "sigmas"):
        assert not (out[k] == fill).any(), k
    assert (out["nits"] > 0).all() and (out["nfevs"] == out["nits"] * P).all() and (out["statuses"] != 77).all()
    return out


def generation_one(fit_of, lower, upper, P, seed, x0, sigma, muperc=0.5):
    """A run with maxiter = 1, plainly: the candidates as the reference forms them from the oracle's own normals, the fitness
    `fit_of(points)` (the test's own, possibly with planted values), numpy's STABLE argsort (lower index first on ties; NaN
    last).  Returns order, fit, the best row un-standardised, the new mean (standardised, summed in np.longdouble)."""
    import oracle

    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    n = len(lower)
    xm, xstd = 0.5 * (upper + lower), 0.5 * (upper - lower)
    stream = oracle.PhiloxStream(seed)
    xmean0 = stream.cma_initial_mean(n) if x0 is None else (np.asarray(x0, dtype=np.float64) - xm) / xstd
    vvec = stream.vd_initial_direction(n) / np.sqrt(n)
    norm_v2 = np.dot(vvec, vvec)
    vn = vvec / np.sqrt(norm_v2)
    arz = stream.cma_normals(1, P, n)
    ary = np.ones(n) * (arz + (np.sqrt(1.0 + norm_v2) - 1.0) * np.outer(np.dot(arz, vn), vn))
    arx = xmean0 + sigma * ary
    with np.errstate(over="ignore", invalid="ignore"):
        fit = fit_of(arx * xstd + xm)
    order = np.argsort(fit, kind="stable")
    mu = int(muperc * P)
    w = np.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
    w /= w.sum()
    L = np.longdouble
    dx = (w.astype(L)[:, None] * arx[order[:mu]].astype(L)).sum(axis=0) - w.astype(L).sum() * xmean0.astype(L)
    return dict(order=order, fit=fit, x=arx[order[0]] * xstd + xm, fun=fit[order[0]], xmean=(xmean0.astype(L) + dx).astype(np.float64))
