"""GPU: non-finite objective values.  The reference picks its best row with np.argmin (the FIRST NaN when any value is
NaN, whatever its sign bit; -0.0 ties 0.0, the lower index wins), ranks with np.argsort (NaN last), takes the swarm radius
with np.max (NaN propagates) and re-seeds the CPSO restart's `pbestfit.argsort()[: -nw - 1 : -1]` (NaN particles first).
The kernels' reductions against those rules, then whole runs with NaN / inf in the population against the oracle."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65537, 131075]
KINDS = ["nan_before", "nan_after", "nan_far", "all_nan", "neg_nan", "inf", "all_inf", "ties", "zeros"]
NEG_NAN = np.frombuffer(np.uint64(0xFFF8000000000000).tobytes(), dtype=np.float64)[0]
POS_NAN = np.frombuffer(np.uint64(0x7FF8000000000001).tobytes(), dtype=np.float64)[0]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@pytest.fixture(scope="module")
def ctx(sa):
    from stochopy_amd import _device

    return _device.Context()


def bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def fitness(P, kind, rs):
    f = rs.uniform(1.0, 2.0, P)
    j = int(rs.randint(P))  # the finite minimum
    f[j] = 0.5
    if kind == "nan_before":
        f[rs.randint(j + 1)] = POS_NAN if j else f[0]
        if j == 0:
            f[0] = POS_NAN
    elif kind == "nan_after":
        f[j + 1 if j + 1 < P else j] = POS_NAN
    elif kind == "nan_far":  # in another workgroup's record (256 rows per workgroup), or past a partial last trip
        f[(j + 300 + P // 2) % P] = POS_NAN
    elif kind == "all_nan":
        f[:] = np.where(rs.rand(P) < 0.5, NEG_NAN, POS_NAN)
    elif kind == "neg_nan":  # numpy's inf - inf on x86: sign bit set; a positive NaN further on must not win
        k = (j + P // 3) % P
        f[k] = NEG_NAN
        f[(k + 1) % P] = POS_NAN if (k + 1) % P != k else f[k]
    elif kind == "inf":
        f[rs.rand(P) < 0.1] = np.inf
        f[(j + 7 * P // 11) % P] = -np.inf
        f[(j + 3 * P // 5) % P] = -np.inf
    elif kind == "all_inf":
        f[:] = np.inf
    elif kind == "ties":  # the minimum in many rows, across records and workgroups
        f = np.floor(rs.rand(P) * 4.0)
    elif kind == "zeros":
        f[rs.rand(P) < 0.01] = 0.0
        f[rs.rand(P) < 0.01] = -0.0
        f[j] = -0.0 if P % 2 else 0.0
        f[(j + P // 2) % P] = 0.0 if P % 2 else -0.0
    return f


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", SIZES)
def test_argmin_kernel_vs_numpy(sa, ctx, P, kind):
    """sx_argmin (grid of 256-row workgroups -> records -> one workgroup) against np.argmin: index and value bits."""
    from stochopy_amd import _device

    t = _device.torch()
    rs = np.random.RandomState(P * 7 + len(kind))
    f = fitness(P, kind, rs)
    want = int(np.argmin(f))
    p = _device.ptr
    ws_len = 1024
    d_f = ctx.upload(f)
    ws_f, ws_i = ctx.zeros((ws_len,)), ctx.zeros((ws_len,), dtype=t.int64)
    out_i, out_f = ctx.zeros((1,), dtype=t.int64), ctx.zeros((1,))
    with t.cuda.stream(ctx.stream):
        rc = ctx.L.sx_argmin(p(d_f), P, p(ws_f), p(ws_i), ws_len, p(out_i), p(out_f), ctx.stream_ptr)
    assert rc == 0
    ctx.sync()
    got_i, got_f = int(out_i.cpu().numpy()[0]), out_f.cpu().numpy()
    assert got_i == want, (kind, P, got_i, want, f[got_i], f[want])
    assert bits(got_f)[0] == bits(f[want]), (kind, P, hex(int(bits(got_f)[0])), hex(int(bits(f[want]))))


# --------------------------------------------------------------------------- #
# whole runs: a NaN / inf in the population, against the oracle (Philox draws)
# --------------------------------------------------------------------------- #
def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(
        np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))


def population(P, n, lo, hi, seed, form):
    x0 = np.random.RandomState(seed).uniform(lo, hi, (P, n))
    if form == "nan":  # NaN in a row before the finite minimum's
        x0[5, 2] = np.nan
    elif form == "nan_late":  # ... and after it
        x0[P - 1, 0] = np.nan
    elif form == "inf":  # +inf and -inf entries: rosenbrock of either is NaN or +inf
        x0[3, 1] = np.inf
        x0[P - 2, n - 1] = -np.inf
    return x0


def check_run(got, ref, history=False):
    assert (got.nit, got.nfev, got.status, got.success) == (ref.nit, ref.nfev, ref.status, ref.success)
    assert same(got.fun, ref.fun), (got.fun, ref.fun)
    assert same(got.x, ref.x), (got.x, ref.x)
    if history:
        assert same(got.funall, ref.funall)
        assert same(got.xall, ref.xall)


RUNS = [("de", "best1bin", "deferred"), ("de", "rand1bin", "deferred"), ("de", "best1bin", "immediate"),
        ("de", "rand1bin", "immediate"), ("pso", None, "deferred"), ("cpso", None, "deferred"), ("pso", None, "immediate")]


@pytest.mark.parametrize("form", ["nan", "nan_late", "inf"])
@pytest.mark.parametrize("run", RUNS, ids=lambda r: "-".join(str(v) for v in r if v))
def test_fused_objective_run_with_nonfinite_x0(sa, run, form):
    """Rosenbrock (fused kernels) from an x0 with a NaN / inf entry: the best row is the first NaN, the run never replaces
    it and ends at maxiter with x = that row, fun = nan; CPSO's radius is NaN, so no restart fires -- the chained
    one-kernel paths (no callback) and the immediate sweeps."""
    method, strategy, updating = run
    n, P, lo, hi = 4, 12, -2.0, 2.0
    opts = {"maxiter": 20, "popsize": P, "seed": 1, "updating": updating}
    if strategy:
        opts["strategy"] = strategy
    x0 = population(P, n, lo, hi, 3, form)
    bounds = [[lo, hi]] * n
    ref = oracle.minimize("rosenbrock", bounds, x0=x0.copy(), method=method, options=dict(opts), rng="philox")
    got = sa.optimize.minimize(sa.factory.rosenbrock, bounds, x0=x0.copy(), method=method,
                               options=dict(opts, backend="hip", rng="philox"))
    check_run(got, ref)
    if form != "inf":  # (rosenbrock of an inf entry is +inf: that row just loses)
        assert np.isnan(got.fun) and got.status == -1


@pytest.mark.parametrize("method", ["de", "pso", "cpso"])
def test_nonfinite_run_with_callback_and_history(sa, method):
    """The two-kernel path (a callback and return_all at verbosity 0: the best row of every generation)."""
    n, P, lo, hi = 5, 16, -2.0, 2.0
    opts = {"maxiter": 15, "popsize": P, "seed": 4, "updating": "deferred", "return_all": True, "verbosity": 0.0}
    x0 = population(P, n, lo, hi, 9, "nan_late")
    bounds = [[lo, hi]] * n
    seen_ref, seen_got = [], []
    ref = oracle.minimize("rosenbrock", bounds, x0=x0.copy(), method=method, options=dict(opts), rng="philox",
                          callback=lambda X, r: seen_ref.append(float(r.fun)))
    got = sa.optimize.minimize(sa.factory.rosenbrock, bounds, x0=x0.copy(), method=method,
                               options=dict(opts, backend="hip", rng="philox"), callback=lambda X, r: seen_got.append(float(r.fun)))
    check_run(got, ref, history=True)
    assert same(seen_got, seen_ref)


@pytest.mark.parametrize("method", ["de", "pso"])
def test_nonfinite_wide_rows(sa, method):
    """Wide rows (n = 3000: the row-per-workgroup kernels) with a NaN row."""
    n, P, lo, hi = 3000, 32, -2.0, 2.0
    opts = {"maxiter": 6, "popsize": P, "seed": 2, "updating": "deferred"}
    x0 = population(P, n, lo, hi, 5, "nan")
    bounds = [[lo, hi]] * n
    ref = oracle.minimize("sphere", bounds, x0=x0.copy(), method=method, options=dict(opts), rng="philox")
    got = sa.optimize.minimize(sa.factory.sphere, bounds, x0=x0.copy(), method=method,
                               options=dict(opts, backend="hip", rng="philox"))
    check_run(got, ref)


def _sum4(T):
    """row sums in one fixed order, so numpy and torch give the same bits"""
    s = T[:, 0] + T[:, 1]
    for j in range(2, T.shape[1]):
        s = s + T[:, j]
    return s


def slab_np(X):
    """sphere around -0.5, NaN where x0 > 1 or x2 > 1.5 (slabs of the domain), -inf on a thin sliver: a caller's objective."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    f = _sum4((X + 0.5) ** 2)
    f = np.where((X[:, 0] > 1.0) | (X[:, 2] > 1.5), np.nan, f)
    return np.where(X[:, 1] < -1.95, -np.inf, f)


def slab_torch(X):
    import torch

    f = _sum4((X + 0.5) ** 2)
    f = torch.where((X[:, 0] > 1.0) | (X[:, 2] > 1.5), torch.full_like(f, float("nan")), f)
    return torch.where(X[:, 1] < -1.95, torch.full_like(f, float("-inf")), f)


def plateau_np(X):
    """the minimum is a plateau: zero on the box |x| <= 0.5 (-0.0 where x0 < 0, 0.0 elsewhere), the squared excess outside."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    d = np.maximum(np.abs(X) - 0.5, 0.0)
    f = _sum4(d * d)
    return np.where((X[:, 0] < 0.0) & (f == 0.0), -0.0, f)


def plateau_torch(X):
    import torch

    d = torch.clamp(X.abs() - 0.5, min=0.0)
    f = _sum4(d * d)
    return torch.where((X[:, 0] < 0.0) & (f == 0.0), torch.full_like(f, -0.0), f)


@pytest.mark.parametrize("objective", ["slab", "plateau"])
@pytest.mark.parametrize("route", ["batched", "serial", "threading"])
@pytest.mark.parametrize("method", ["de", "pso", "cpso", "na"])
def test_caller_objective_with_nonfinite_values(sa, method, route, objective):
    """A caller's objective that returns NaN / -inf on part of the domain, or a plateau of tied minima with -0.0 and 0.0:
    factory.batched, a plain Python callable serially, and through the threading host pool."""
    n, P = 4, 16
    bounds = [[-2.0, 2.0]] * n
    opts = {"maxiter": 12, "popsize": P, "seed": 6, "return_all": True, "verbosity": 0.0}
    if method != "na":
        opts["updating"] = "deferred"
    fnp, ftorch = (slab_np, slab_torch) if objective == "slab" else (plateau_np, plateau_torch)
    ref = oracle.minimize(fnp, bounds, method=method, options=dict(opts), rng="philox")
    if route == "batched":
        fun, extra = sa.factory.batched(ftorch), {}
    else:
        fun = lambda x: float(fnp(x)[0])  # noqa: E731
        extra = {"host_workers": 3, "host_backend": "threading"} if route == "threading" else {}
    got = sa.optimize.minimize(fun, bounds, method=method, options=dict(opts, backend="hip", rng="philox", **extra))
    check_run(got, ref, history=True)
    assert bits(got.fun) == bits(ref.fun) or (np.isnan(got.fun) and np.isnan(ref.fun))


@pytest.mark.parametrize("kind", ["nan_before", "nan_far", "neg_nan", "all_nan", "inf", "all_inf", "ties", "zeros"])
@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 257, 4097, 5000])
def test_cma_rank_kernel_vs_numpy(sa, ctx, P, kind):
    """The ranking launch of the device-resident CMA-ES / VD-CMA generations (sx_cma_rank = cma_rank_launch): order is
    np.argsort(kind="stable") -- NaN last, ties by lower index -- best_row / fbest / the best-f history are order[0]'s,
    and the return_all entry with 0 rows (state.reserved[5]) is np.argmin's: the first NaN when there is one."""
    from stochopy_amd import _device, _lib

    t = _device.torch()
    p = _device.ptr
    f = fitness(P, kind, np.random.RandomState(P * 3 + len(kind)))
    gen = 2
    st = _lib.SxCmaState(it=1, nfev=0, best_row=-1, fbest=0.0, sigma=1.0, sigma_next=1.0, tmp_coef=0.0, psnorm=0.0,
                         status=_lib.SX_STATUS_NONE, done=0, stop_it=0)
    st.reserved[5] = -1.0
    d_state = ctx.upload(np.frombuffer(bytes(st), dtype=np.int64).copy())
    d_f, order, besthist = ctx.upload(f), ctx.zeros((P,), dtype=t.int64), ctx.zeros((4,))
    with t.cuda.stream(ctx.stream):
        rc = ctx.L.sx_cma_rank(p(d_f), P, p(order), p(d_state), p(besthist), gen, ctx.stream_ptr)
    assert rc == 0
    ctx.sync()
    want = np.argsort(f, kind="stable")
    got = order.cpu().numpy()
    assert np.array_equal(got, want), (kind, P, np.flatnonzero(got != want)[:8])
    s = _lib.SxCmaState.from_buffer_copy(d_state.cpu().numpy().tobytes())
    assert s.best_row == want[0] and bits(s.fbest) == bits(f[want[0]])
    assert bits(besthist.cpu().numpy()[gen - 1]) == bits(f[want[0]])
    assert int(s.reserved[5]) == int(np.argmin(f)), (kind, P, s.reserved[5], np.argmin(f))


@pytest.mark.parametrize("method", ["cmaes", "vdcma"])
@pytest.mark.parametrize("verbosity", [0.0, 0.5])
def test_cma_host_loop_with_nan_slab(sa, method, verbosity):
    """CMA-ES / VD-CMA (host-driven loop: a caller's objective) with a NaN slab that some candidates of the run hit (never
    more than P - mu in a generation: the model stays finite, as in the reference): argsort puts them last, the history
    entry with 0 rows is argmin's."""
    n, P = 6, 20
    bounds = [[-3.0, 3.0]] * n
    opts = {"maxiter": 25, "popsize": P, "seed": 12, "sigma": 0.5, "return_all": True, "verbosity": verbosity}
    hits = []

    def probe(it, before, after):
        model = after["C"] if "C" in after else after["dvec"]
        hits.append((int(np.isnan(after["arfit"]).sum()), bool(np.isfinite(model).all())))

    def slab(X):
        X = np.atleast_2d(X)
        f = ((X - 0.3) ** 2).sum(axis=1)
        return np.where(X[:, 0] > 0.9, np.nan, f)

    def slab_t(X):
        import torch

        f = ((X - 0.3) ** 2).sum(dim=1)
        return torch.where(X[:, 0] > 0.9, torch.full_like(f, float("nan")), f)

    o = dict(opts, eigh="canonical") if method == "cmaes" else dict(opts)
    o.pop("seed")
    lower, upper = np.transpose(np.asarray(bounds, dtype=np.float64))
    ref = oracle.engine.RUNNERS[method](slab, lower, upper, None, oracle.engine.make_stream("philox", opts["seed"]),
                                        probe=probe, **o)
    assert any(k > 0 for k, _ in hits), "the slab is never hit: the case tests nothing"
    assert all(k <= P - P // 2 and ok for k, ok in hits), hits
    got = sa.optimize.minimize(sa.factory.batched(slab_t), bounds, method=method, options=dict(opts, backend="hip", rng="philox"))
    assert (got.nit, got.status) == (ref.nit, ref.status)
    assert got.funall.shape == ref.funall.shape
    assert np.array_equal(np.isnan(got.funall), np.isnan(ref.funall))
    assert np.allclose(got.funall, ref.funall, rtol=1e-6, equal_nan=True)
    assert np.allclose(got.xall, ref.xall, rtol=1e-6, atol=1e-9, equal_nan=True)
    assert np.isclose(got.fun, ref.fun, rtol=1e-6)


@pytest.mark.parametrize("form", ["inf", "nan"])
@pytest.mark.parametrize("path", ["chained", "two_kernel"])
def test_long_cpso_run_with_nonfinite_x0(sa, path, form):
    """CPSO over 200 generations from an x0 with a NaN / inf entry (the oracle pinned to the reference's
    cpso_long_* fixtures): np.max of the radii propagates NaN, so restarts fire exactly where the oracle's do."""
    n, P, lo, hi = 4, 12, -2.0, 2.0
    opts = {"maxiter": 200, "popsize": P, "seed": 1, "updating": "deferred"}
    if path == "two_kernel":
        opts.update(return_all=True, verbosity=0.0)
    x0 = population(P, n, lo, hi, 3, form)
    bounds = [[lo, hi]] * n
    seen_ref, seen_got = [], []
    cb = (lambda X, r: seen_ref.append(float(r.fun))) if path == "two_kernel" else None
    ref = oracle.minimize("rosenbrock", bounds, x0=x0.copy(), method="cpso", options=dict(opts), rng="philox", callback=cb)
    cb = (lambda X, r: seen_got.append(float(r.fun))) if path == "two_kernel" else None
    got = sa.optimize.minimize(sa.factory.rosenbrock, bounds, x0=x0.copy(), method="cpso",
                               options=dict(opts, backend="hip", rng="philox"), callback=cb)
    check_run(got, ref, history=path == "two_kernel")
    assert same(seen_got, seen_ref)


@pytest.mark.parametrize("method", ["pso", "cpso"])
def test_pso_kernel_nan_in_a_later_wave(sa, method):
    """The PSO generation (n = 4 * LPR = 64) with more than 64 workgroups, so the records spread over several waves of
    the finalising workgroup: a NaN row in the last records (a later wave) must beat the finite minimum in wave 0's
    records."""
    from stochopy_amd import _device

    L = _device.Context().L
    n, P = 64, 8192
    rpw = int(L.sx_rows_per_workgroup(n))
    assert (P + rpw - 1) // rpw > 2 * 64  # records in three or more waves
    x0 = np.random.RandomState(8).uniform(-2.0, 2.0, (P, n))
    x0[2] = 0.9  # the finite minimum: record 0, wave 0
    x0[P - 3, 7] = np.nan  # the last record: a later wave
    bounds = [[-2.0, 2.0]] * n
    opts = {"maxiter": 6, "popsize": P, "seed": 3, "updating": "deferred"}
    ref = oracle.minimize("rosenbrock", bounds, x0=x0.copy(), method=method, options=dict(opts), rng="philox")
    got = sa.optimize.minimize(sa.factory.rosenbrock, bounds, x0=x0.copy(), method=method,
                               options=dict(opts, backend="hip", rng="philox"))
    check_run(got, ref)
    assert np.isnan(got.fun) and same(got.x, x0[P - 3])
