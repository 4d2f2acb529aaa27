"""The batched-runs CMA-ES kernel (csrc/sx_cma_runs.hip) for the tests: the LDS layout the kernel's header comment documents,
restated in bytes; launch_runs, the batch optimize.minimize(runs=R) launches (optimize/_cmaes.py _runs_batch) but with real
nfevs / xmeans buffers (minimize() passes nfevs = xmeans = NULL); generation_one, a plain numpy reference of a run's first
generation; and the shapes the generation-1 tests share.  A plain helper module (imported, not collected)."""

import numpy as np

from _runs_abi import FILL, largest, launch_filled

LDS_LIMIT = 160 * 1024
MAX_DIM = 32


def solver_size(n):
    """M2 of the one-workgroup Jacobi solver that serves dimension n."""
    return 16 if n <= 16 else 32


def lds_bytes(P, n):
    """C[n][ldn] | B[n][ldn] | nine vectors of n | lam, scl, inv [M2] each | fit[P] | order[P] as int32 | red[24] | part[8][4] |
    max(candidates P * (n + 8), Jacobi storage 4 * M2 * (M2 + 1) + 2 * M2), in bytes; ldn = n | 1."""
    ldn, m2 = n | 1, solver_size(n)
    fixed = 2 * n * ldn + 9 * n + 3 * m2 + P + (P + 1) // 2 + 24 + 32
    return 8 * (fixed + max(P * (n + 8), 4 * m2 * (m2 + 1) + 2 * m2))


def workspace_bytes(R, maxiter):
    """One zero-initialised best-fitness history of maxiter doubles per run."""
    return 8 * R * maxiter


def largest_popsize(lib, n):
    """The largest P with sx_cma_runs_lds_bytes(P, n) > 0 (the function refuses everything above it)."""
    return largest(lambda p: lib.sx_cma_runs_lds_bytes(p, n) > 0, 2, 1 << 20)


def jacobi_doubles(n):
    """The solver's storage that shares the region U with the candidates: S[2], W[2] of [M2][M2 + 1], c[M2], s[M2]."""
    m2 = solver_size(n)
    return 4 * m2 * (m2 + 1) + 2 * m2


def crossover_popsize(n):
    """The largest P whose candidates P * (n + 8) are NOT larger than the Jacobi storage: P and P + 1 are the two sides."""
    return jacobi_doubles(n) // (n + 8)


def largest_popsize_below(limit_bytes, n):
    """The largest P with lds_bytes(P, n) <= limit_bytes (lds_bytes never decreases in P)."""
    P = 2
    while lds_bytes(P + 1, n) <= limit_bytes:
        P += 1
    return P


def standardise(lower, upper):
    """xm, xstd of cmaes/_cmaes.py:164-165."""
    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    return 0.5 * (upper + lower), 0.5 * (upper - lower)


def launch_runs(objective, lower, upper, P, seeds, x0=None, maxiter=100, sigma=0.1, muperc=0.5, xtol=1e-8, ftol=1e-8):
    """One sx_cma_runs_launch of len(seeds) runs of `objective` (a factory name): the batch minimize() launches
    (optimize/_cmaes.py _runs_batch), with real nfevs / xmeans buffers.  lower / upper: one value per dimension.  x0: None
    (every run draws its initial mean as the single run of its seed does), (n,) or (R, n), in the caller's coordinates.
    Returns xs (R, n), funs (R,), nits (R,), statuses (R,), nfevs (R,), sigmas (R,), xmeans (R, n; standardised)."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize._cmaes import _runs_batch

    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    batch = _runs_batch([int(s) for s in seeds], _lib.FUN_IDS[objective], lower, upper, x0, maxiter, P, sigma, muperc, xtol,
                        ftol, outputs=("nfevs", "xmeans"))
    # filled with values no run produces: an element the kernel does not write cannot pass for a result
    fills = dict(dict.fromkeys(("xs", "funs", "sigmas", "xmeans"), FILL), nits=-7, nfevs=-7, statuses=77)
    out = launch_filled(batch, fills)
    out = tuple(out[k] for k in ("xs", "funs", "nits", "statuses", "nfevs", "sigmas", "xmeans"))
    assert not (out[0] == FILL).any() and not (out[6] == FILL).any() and not (out[5] == FILL).any()
    assert (out[2] > 0).all() and (out[4] > 0).all() and (out[3] != 77).all()
    return out


def generation_one(objective, lower, upper, P, seed, x0, sigma=0.1, muperc=0.5):
    """A run with maxiter = 1, plainly: one generation from the identity model (C = B = I, D = 1, ps = 0), so
    invsqrtC (xmean - xold) is the step itself.  The candidates are formed as the reference forms them (doubles, one product
    and one sum per element), ranked by numpy's STABLE argsort (lower index first on ties; NaN last), and every sum -- the
    recombination and |ps|^2 -- is accumulated in np.longdouble.  Returns a dict: arx (P, n), fit, order, xmean (standardised),
    absum (the sum_k |w_k arx_k| the error bound of xmean is stated in), sigma (after the generation), x (the best row,
    un-standardised), xparts (|arx xstd| + |xm| of that row: the magnitude its multiply-add works at), fun, nit, nfev, status,
    mu, sigma_sens (d sigma / d |xmean|: |ps| is kps |xmean - xmean0| / sigma, and sigma' = sigma exp((cs / damps)(|ps| / chind - 1)))."""
    import oracle
    from oracle.engine import cma_constants

    lower, upper = np.asarray(lower, dtype=np.float64), np.asarray(upper, dtype=np.float64)
    n = len(lower)
    xm, xstd = standardise(lower, upper)
    k = cma_constants(n, P, muperc)
    mu, w = k["mu"], k["w"]
    stream = oracle.PhiloxStream(seed)
    xmean0 = stream.cma_initial_mean(n) if x0 is None else (np.asarray(x0, dtype=np.float64) - xm) / xstd
    Z = stream.cma_normals(1, P, n)
    arx = xmean0 + sigma * Z
    with np.errstate(over="ignore", invalid="ignore"):
        fit = oracle.evaluate(objective, arx * xstd + xm)
    order = np.argsort(fit, kind="stable")
    L = np.longdouble
    sel = arx[order[:mu]].astype(L)
    terms = w.astype(L)[:, None] * sel
    xmean = terms.sum(axis=0)
    absum = np.abs(terms).sum(axis=0)
    ps = L(np.sqrt(k["cs"] * (2.0 - k["cs"]) * k["mueff"])) * (xmean - xmean0.astype(L)) / L(sigma)
    psn = np.sqrt((ps * ps).sum())
    sigma1 = L(sigma) * np.exp(L(k["cs"] / k["damps"]) * (psn / L(k["chind"]) - L(1.0)))
    best = int(order[0])
    return dict(arx=arx, fit=fit, order=order, xmean=xmean.astype(np.float64), absum=absum.astype(np.float64),
                sigma=float(sigma1), x=arx[best] * xstd + xm, xparts=np.abs(arx[best] * xstd) + np.abs(xm), fun=float(fit[best]),
                nit=1, nfev=P, status=-1, mu=mu,
                sigma_sens=float(sigma1) * k["cs"] / k["damps"] / k["chind"] * np.sqrt(k["cs"] * (2.0 - k["cs"]) * k["mueff"]) / sigma)


# ---- the generation-1 cases of tests/test_gpu_cma_runs_edges.py, shared with the host check of the reference
# (tests/test_cma_runs_host.py).  (n, P): P at the LDS limit of n, each side of 64 KiB of LDS (where the launch raises the
# kernel's dynamic-LDS attribute), each side of the candidates | Jacobi-storage cross-over of the shared region U.
GEN1_LITERALS = [(1, 2), (1, 1939), (16, 46), (16, 47), (16, 290), (16, 291), (16, 772), (17, 171), (17, 172), (17, 739),
                 (32, 107), (32, 108), (32, 135), (32, 136), (32, 432)]
# sigma = 2^-10: sigma * z is exact, so `xmean0 + sigma * z` is ONE rounding whether or not the device contracts it to an fma;
# and the few ulp by which the device's log / sincos differ from libm's in z arrive at a candidate scaled by 2^-10 |z| / |arx|.
GEN1_SIGMA = 2.0 ** -10


def gen1_shapes(lib):
    """The shapes above from the library's own budget (largest_popsize, lds_bytes), not from the literals."""
    shapes = [(1, 2), (1, largest_popsize(lib, 1))]
    for n in (16, 17, 32):
        x, k = crossover_popsize(n), largest_popsize_below(64 * 1024, n)
        shapes += [(n, x), (n, x + 1)]
        if n != 17:
            shapes += [(n, k), (n, k + 1)]
        shapes.append((n, largest_popsize(lib, n)))
    return shapes


def gen1_box(n):
    """Per dimension and asymmetric: no centre is 0, no two half-widths are equal."""
    i = np.arange(n, dtype=np.float64)
    return -1.0 - i / 7.0, 2.0 + i / 3.0


def gen1_x0(n, R):
    """A point per run, inside the box, in its upper half (standardised mean 0.1 ... 0.9 per element: a candidate is not a
    difference of nearly equal numbers)."""
    lower, upper = gen1_box(n)
    r, i = np.arange(R)[:, None], np.arange(n)[None, :]
    frac = 0.55 + 0.4 * ((7 * r + 3 * i) % 11) / 11.0
    return lower + (upper - lower) * frac
