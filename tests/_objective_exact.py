"""The seven objectives restated in np.longdouble, their inputs on each objective's own domain and at the arguments where a
hand-written cosine goes wrong, and the bound the device's values are held to (tests/test_gpu_objective_domains.py; the
restatement itself is checked on the CPU by tests/test_objective_exact_host.py).  A plain helper module; numpy only.

What is restated is the FUNCTION, not numpy's rounding of it: cos(2 pi x) is taken as cos(2 pi_ld (x - rint(x))) -- the
reduction is exact in double and the period is 1 -- where numpy (and the reference) take the cosine of the ROUNDED product
2 pi x.  The doubles that are part of the function stay doubles, as in tests/_sample_edges.py: griewank's x / sqrt(j + 1),
the literal e, 0.2 and 39.16599.
"""
import functools

import numpy as np

from oracle.objectives import OBJECTIVES

LD = np.longdouble
ALL = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")
COS_2PI = ("ackley", "rastrigin")             # the objectives whose terms go through cos_2pi (csrc/sx_device.hpp)
COSINE = ("ackley", "griewank", "rastrigin")  # a non-finite element gives NaN
BIT_EQUAL = ("rosenbrock", "sphere")          # + - * only, in numpy's order: the device's values are numpy's bits
DOMAIN = {"ackley": 32.768, "griewank": 600.0, "quartic": 1.28, "styblinski_tang": 5.0, "rastrigin": 5.12,
          "rosenbrock": 5.12, "sphere": 5.12}
WIDE = 600.0
NS = (1, 2, 3, 7, 64, 300)
ROWS = 64
HUGE = 2.0 ** 52  # from here on a double is an integer: cos(2 pi x) is exactly 1
EPS = 2.0 ** -52
FACTOR = {name: 4.0 for name in ALL}  # the device's cos / exp / sqrt need not be correctly rounded where glibc's mostly are

PI_LD = LD("3.14159265358979323846264338327950288")
E_DOUBLE = 2.7182818284590451


def have_longdouble():
    return np.finfo(LD).nmant >= 63


def cos_2pi(X):
    """cos(2 pi x), exact reduction: (P, n) float64 -> longdouble."""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y = X - np.rint(X)  # exact (Sterbenz for |x| >= 1/2, x itself below); inf - inf = NaN
    return np.cos((2 * PI_LD) * y.astype(LD))


def exact(name, X):
    """The objective of every row of X, (P, n) float64, in np.longdouble."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[1]
    x = X.astype(LD)
    j = np.arange(1, n + 1)
    with np.errstate(all="ignore"):
        if name == "ackley":
            s1 = np.sqrt((x * x).sum(axis=1) / n)
            s2 = cos_2pi(X).sum(axis=1) / n
            return (LD(20.0) + LD(E_DOUBLE)) - 20 * np.exp(-LD(0.2) * s1) - np.exp(s2)
        if name == "griewank":
            arg = X / np.sqrt(j.astype(np.float64))  # the double quotient is the function's argument
            return 1 + (x * x).sum(axis=1) / 4000 - np.prod(np.cos(arg.astype(LD)), axis=1)
        if name == "quartic":
            return (j.astype(LD) * (x * x) * (x * x)).sum(axis=1)
        if name == "rastrigin":
            return 10 * LD(n) + (x * x - 10 * cos_2pi(X)).sum(axis=1)
        if name == "rosenbrock":
            head = x[:, :-1]
            t = x[:, 1:] - head * head
            return 100 * (t * t).sum(axis=1) + ((1 - head) * (1 - head)).sum(axis=1)
        if name == "sphere":
            return (x * x).sum(axis=1)
        if name == "styblinski_tang":
            x2 = x * x
            return (x2 * x2 - 16 * x2 + 5 * x).sum(axis=1) / 2 + LD(39.16599) * n
    raise KeyError(name)


def exact_mp(name, row, digits=40):
    """One row at `digits` decimal digits with mpmath (the same function: the same doubles stay doubles)."""
    import mpmath

    with mpmath.workdps(digits):
        mp = mpmath.mpf
        x = [mp(float(v)) for v in row]
        n = len(x)
        c2 = [mpmath.cos(2 * mpmath.pi * (v - mpmath.nint(v))) for v in x]
        if name == "ackley":
            s1 = mpmath.sqrt(sum(v * v for v in x) / n)
            return (mp(20.0) + mp(E_DOUBLE)) - 20 * mpmath.exp(-mp(0.2) * s1) - mpmath.exp(sum(c2) / n)
        if name == "griewank":
            arg = np.asarray(row, dtype=np.float64) / np.sqrt(np.arange(1, n + 1).astype(np.float64))
            p = mp(1)
            for a in arg:
                p *= mpmath.cos(mp(float(a)))
            return 1 + sum(v * v for v in x) / 4000 - p
        if name == "quartic":
            return sum((k + 1) * v ** 4 for k, v in enumerate(x))
        if name == "rastrigin":
            return 10 * n + sum(v * v - 10 * c for v, c in zip(x, c2))
        if name == "rosenbrock":
            return 100 * sum((b - a * a) ** 2 for a, b in zip(x, x[1:])) + sum((1 - a) ** 2 for a in x[:-1])
        if name == "sphere":
            return sum(v * v for v in x)
        if name == "styblinski_tang":
            return sum(v ** 4 - 16 * v * v + 5 * v for v in x) / 2 + mp(39.16599) * n
    raise KeyError(name)


def kernel_association(name, X):
    """quartic and styblinski_tang with the kernel's x^4 = (x x)(x x) (csrc/sx_device.hpp) in place of np.power's correctly
    rounded one, otherwise oracle.objectives' expression and numpy's pairwise sum: the bits the device gives."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    n = X.shape[1]
    X2 = X * X
    if name == "quartic":
        return (np.arange(1, n + 1) * (X2 * X2)).sum(axis=1)
    if name == "styblinski_tang":
        return 0.5 * ((X2 * X2 - 16.0 * X2) + 5.0 * X).sum(axis=1) + 39.16599 * n
    raise KeyError(name)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _near(v):
    v = np.float64(v)
    return [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]


@functools.lru_cache(maxsize=None)
def planted_values():
    """The arguments a hand-written cos(2 pi x) has to get right: signed zeros, integers, half and quarter integers up to
    600 with their neighbours one ulp away, the tiniest numbers, and doubles that are integers by their size."""
    ks = (0, 1, 2, 3, 4, 5, 7, 31, 32, 33, 100, 255, 256, 511, 512, 599, 600)
    out = [0.0, -0.0, 1.0e-300, -1.0e-300, 5.0e-324, -5.0e-324]
    for k in ks:
        for s in (1.0, -1.0):
            for v in (k, k + 0.5, k - 0.5, k + 0.25, k - 0.25):
                out += _near(s * v)
    out += [HUGE, -HUGE, 2.0 ** 53 + 2.0, -(2.0 ** 53 + 2.0)]
    v = np.array(out, dtype=np.float64)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def rows(name, n, kind):
    """(rows, n) float64, read-only.  kind: "own" -- uniform in the objective's own domain; "wide" -- uniform in +-600;
    "planted" (the cos_2pi objectives) -- n = 1: every planted value a row; longer rows: own-domain rows with planted values
    (|x| < 2^52) at a few places each, and behind them rows that hold one of the huge values."""
    rs = np.random.RandomState(7919 * n + 31 * ALL.index(name) + {"own": 0, "wide": 1, "planted": 2}[kind])
    if kind in ("own", "wide"):
        lim = DOMAIN[name] if kind == "own" else WIDE
        X = rs.uniform(-lim, lim, (ROWS, n))
    else:
        v = planted_values()
        if n == 1:
            X = v[:, None].copy()
        else:
            small, huge = v[np.abs(v) < HUGE], v[np.abs(v) >= HUGE]
            per = min(n, 3)
            nrows = -(-small.size // per)
            X = rs.uniform(-DOMAIN[name], DOMAIN[name], (nrows + huge.size, n))
            order = rs.permutation(small.size)
            for r in range(nrows):
                take = small[order[r * per:(r + 1) * per]]
                X[r, rs.choice(n, take.size, replace=False)] = take
            for r, h in enumerate(huge):
                X[nrows + r, rs.randint(n)] = h
    X.setflags(write=False)
    return X


def nonfinite_rows(name, n):
    """Own-domain rows with a NaN, +inf or -inf at one place each (first, last and a middle element)."""
    rs = np.random.RandomState(101 * n + ALL.index(name))
    X = rs.uniform(-DOMAIN[name], DOMAIN[name], (9, n))
    for r, bad in enumerate((np.nan, np.inf, -np.inf) * 3):
        X[r, (0, n - 1, n // 2)[r // 3]] = bad
    return X


def kinds(name):
    return ("own", "wide", "planted") if name in COS_2PI else ("own", "wide")


# ---- the bound -------------------------------------------------------------------------------------------------------------
def huge_rows(X):
    return np.any(np.abs(X) >= HUGE, axis=1)


def argument_term(name, X):
    """A: what the reference's rounding of the ARGUMENT 2 pi x may move the objective by, as csrc/sx_device.hpp documents
    for cos_2pi (the device reduces exactly and owes none of it; numpy's value carries it)."""
    ok = ~huge_rows(X)
    if name not in COS_2PI or not ok.any():
        return 0.0
    arg = 2.0 * np.pi * float(np.abs(X[ok]).max())
    return (10.0 * X.shape[1] if name == "rastrigin" else np.e) * arg * EPS


def measure(name, X, device):
    """Against the long-double value of every row: E, numpy's own error max |numpy - exact| / max(1, |exact|) over the rows
    below 2^52; the bound 4 max(E, 2^-52) max(1, |exact|) + A per row (rows beyond 2^52: the cosine is exactly 1 and numpy's
    rounded argument means nothing -- 4 * 2^-52 max(1, |exact|)); and the device's error as a fraction of that bound, per row."""
    ref = exact(name, X)
    scale = np.maximum(1.0, np.abs(ref)).astype(LD)
    big = huge_rows(X)
    with np.errstate(all="ignore"):
        host = OBJECTIVES[name](X)
    E = float(np.max(np.abs(host[~big].astype(LD) - ref[~big]) / scale[~big])) if (~big).any() else 0.0
    bound = np.where(big, FACTOR[name] * EPS * scale, FACTOR[name] * max(E, EPS) * scale + argument_term(name, X))
    err = np.abs(np.asarray(device, dtype=np.float64).astype(LD) - ref)
    return E, (err / bound).astype(np.float64), ref
