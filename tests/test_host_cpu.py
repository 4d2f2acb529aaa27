"""CPU-only tests: host RNG replica vs numpy, the C-ABI surface, host-side API logic.

No GPU: these load the shared library (hipcc cross-compiled it) and call only host entry points.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, unhex


@pytest.fixture(scope="module")
def lib():
    from stochopy_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


def test_library_exports_every_declared_symbol(lib):
    """Every function include/stochopy_hip.h declares must resolve in the .so (and be bound in _lib.PROTOTYPES)."""
    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(sx_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 30
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.PROTOTYPES, f"{name} has no ctypes prototype"
    assert set(_lib.PROTOTYPES) <= declared | {"sx_abi_version"}
    assert lib.sx_abi_version() == 1


def test_struct_layouts_match_the_header(lib):
    from stochopy_amd import _lib

    assert C.sizeof(_lib.SxState) == 64 == lib.sx_struct_size(0)
    assert C.sizeof(_lib.SxDeArgs) == lib.sx_struct_size(1)
    assert C.sizeof(_lib.SxPsoArgs) == lib.sx_struct_size(2)
    assert C.sizeof(_lib.SxXchgArgs) == lib.sx_struct_size(3)
    assert C.sizeof(_lib.SxCmaState) == lib.sx_struct_size(4)
    assert C.sizeof(_lib.SxCmaArgs) == lib.sx_struct_size(5)
    assert C.sizeof(_lib.SxVdArgs) == lib.sx_struct_size(6)
    # field offsets of the scalars that follow the pointer block
    assert _lib.SxDeArgs.P.offset == 14 * 8 and _lib.SxDeArgs.key0.offset == C.sizeof(_lib.SxDeArgs) - 8
    assert _lib.SxPsoArgs.P.offset == 14 * 8 and _lib.SxPsoArgs.key0.offset == C.sizeof(_lib.SxPsoArgs) - 8


class Stream:
    def __init__(self, seed):
        from stochopy_amd import _rng

        state = np.random.get_state()
        self.s = _rng.LegacyHostStream(seed)
        np.random.set_state(state)


def test_rng_stream_golden(lib):
    """tests/golden/rng_stream.json: the call sequence captured from numpy's legacy global stream."""
    g = load_golden("rng_stream.json")
    s = Stream(g["seed"]).s
    lo, hi = np.array([-1.0, 0.0, 2.5]), np.array([1.0, 10.0, 2.75])
    for call in g["calls"]:
        name = call["call"]
        if name == "rand(3,4)":
            got = s.random((3, 4)).ravel()
        elif name.startswith("permutation(delete"):
            p = s.permutation(7)
            got = np.delete(np.arange(8), 3)[p]
        elif name == "permutation(8)":
            got = s.permutation(8)
        elif name == "randint(128,size=10)":
            got = s.randint(128, 10)
        elif name == "randint(2)":
            got = s.randint(2, 1)
        elif name == "randint(100,size=7)":
            got = s.randint(100, 7)
        elif name in ("randn(3)",):
            got = s.randn((3,))
        elif name.startswith("uniform(lo,hi,(4,3))"):
            got = s.uniform_rows(lo, hi, 4).ravel()
        elif name == "uniform(-1,1,5)":
            got = s.uniform(-1.0, 1.0, 5)
        elif name == "uniform(size=(2,3))":
            got = s.random((2, 3)).ravel()
        elif name == "uniform(0.25,0.75)":
            got = s.uniform(0.25, 0.75, 1)
        elif name == "normal(0,1,4)":
            got = s.randn((4,))
        elif name.startswith("randint(2**32"):
            got = s.randint(4294967296, 4)
        else:
            raise AssertionError(name)
        want = unhex(call["f64"]) if "f64" in call else np.array(call["i64"])
        assert np.array_equal(np.asarray(got).ravel(), np.asarray(want).ravel()), name
    for entry in g["long"]:
        s = Stream(entry["seed"]).s
        import hashlib

        d = s.random((1000,))
        assert hashlib.sha256(d.tobytes()).hexdigest() == entry["rand1000_sha"]
        z = s.randn((1001,))
        assert hashlib.sha256(z.tobytes()).hexdigest() == entry["randn1001_sha"]
        assert [int(v) for v in s.permutation(257)] == entry["permutation257"]
        r = s.randint(1000, 500)
        assert int(r.sum()) == entry["randint1000x500_sum"]


@pytest.mark.parametrize("seed", [0, 1, 42, 2**32 - 1])
def test_rng_matches_numpy_live(lib, seed):
    """Same draws as numpy.random.RandomState, incl. the DE donor permutations and LHS."""
    s = Stream(seed).s
    rs = np.random.RandomState(seed)
    assert np.array_equal(s.random((5, 7)), rs.rand(5, 7))
    P, k = 37, 5
    don = s.de_donors(P, k)
    ref = np.transpose([rs.permutation(np.delete(np.arange(P), i)) for i in range(P)])[:k]
    assert np.array_equal(don, ref)
    assert np.array_equal(s.randint(13, P), rs.randint(13, size=P))
    lo, hi = np.linspace(-3, -1, 6), np.linspace(1, 4, 6)
    assert np.array_equal(s.uniform_rows(lo, hi, 9), rs.uniform(lo, hi, (9, 6)))
    assert np.array_equal(s.randn((4, 5)), rs.randn(4, 5))  # leaves a cached gaussian
    assert np.array_equal(s.randn((3,)), rs.randn(3))


@pytest.mark.parametrize("P,k,seed,skip", [(256, 2, 1, 0), (300, 5, 2, 7), (1000, 3, 3, 1), (2048, 2, 5, 11), (4096, 2, 0, 5),
                                           (4097, 4, 9, 3), (257, 3, 4, 623)])
@pytest.mark.parametrize("scalar", [False, True, "wide-index"])
def test_large_population_donors_match_numpy(lib, P, k, seed, skip, scalar):
    """de/_de.py:304-311 at population sizes that take the wide form of the donor draws (csrc/sx_mt19937.cpp: masked
    rejection 64 words at a time, the permutation's first k entries by walking the swaps backwards -- no array is
    shuffled): the same donors as numpy's legacy permutation() of every individual's index list, and the stream left at
    the same word (the draws behind it agree).  Both forms (SX_MT_SCALAR=1: the plain replay) in a fresh process each,
    the CPU check is made once per process.  "wide-index" (SX_MT_WIDE_INDEX=1): the 32-bit-index instantiation
    of the wide form -- what populations of more than 65535 individuals (BASELINE config 5 with rng="numpy-legacy") run -- at
    these small sizes, where numpy itself can still be asked."""
    import subprocess
    import sys

    code = f"""
import sys, numpy as np
sys.path.insert(0, {ROOT!r})
from stochopy_amd import _rng
s = _rng.LegacyHostStream({seed})
rs = np.random.RandomState({seed})
if {skip}:
    assert np.array_equal(s.random({skip}), rs.rand({skip}))
got = s.de_donors({P}, {k})
ref = np.empty(({k}, {P}), dtype=np.int32)
idx = np.arange({P})
for i in range({P}):
    ref[:, i] = rs.permutation(np.delete(idx, i))[:{k}]
assert np.array_equal(got, ref), "donors differ"
assert np.array_equal(s.randint(1000, 8), rs.randint(1000, size=8)), "stream position differs"
assert np.array_equal(s.random((3, 5)), rs.rand(3, 5))
print("ok")
"""
    env = dict(os.environ)
    env.pop("SX_MT_SCALAR", None)
    env.pop("SX_MT_WIDE_INDEX", None)
    if scalar == "wide-index":
        env["SX_MT_WIDE_INDEX"] = "1"
    elif scalar:
        env["SX_MT_SCALAR"] = "1"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("P,k,n,bounded", [(9, 3, 1, False), (37, 5, 13, True), (130, 2, 64, True), (40, 4, 5, False)])
def test_async_de_draws_match_numpy(lib, P, k, n, bounded):
    """updating="immediate": per individual donor permutation, randint(ndim), Random's uniform(lower, upper, n)
    (de/_de.py:376-382), against numpy itself and against the oracle's stream."""
    from oracle.streams import LegacyStream

    s = Stream(5).s
    rs = np.random.RandomState(5)
    lo, hi = np.linspace(-3, -1, n), np.linspace(1, 4, n)
    don = np.empty((k, P), dtype=np.int32)
    irand = np.empty(P, dtype=np.int32)
    res = np.empty((P, n)) if bounded else None
    r1 = s.random((P, n))
    s.de_async_draws(P, k, n, don, irand, lo, hi, res)
    assert np.array_equal(r1, rs.rand(P, n))
    for i in range(P):
        assert np.array_equal(don[:, i], rs.permutation(np.delete(np.arange(P), i))[:k])
        assert irand[i] == rs.randint(n)
        if bounded:
            assert np.array_equal(res[i], rs.uniform(lo, hi, n))
    assert np.array_equal(s.random((3,)), rs.rand(3))  # both streams stand at the same place
    d = LegacyStream(5).de_generation_async(2, P, n, k, (lo, hi) if bounded else None)
    assert np.array_equal(d["donors"], don) and np.array_equal(d["irand"], irand) and np.array_equal(d["r1"], r1)
    if bounded:
        assert np.array_equal(d["resample"], res)


def test_rng_global_state_interchange(lib):
    """seed=None continues numpy's global stream; sync_back() hands the advanced state back."""
    from stochopy_amd import _rng

    np.random.seed(123)
    a = np.random.rand(3)
    s = _rng.LegacyHostStream(None)
    b = s.random((4,))
    s.sync_back()
    c = np.random.rand(2)
    np.random.seed(123)
    assert np.array_equal(np.concatenate([a, b, c]), np.random.rand(9))


def test_lhs_matches_oracle(lib):
    import oracle
    from oracle import engine as oe

    lo, hi = np.full(5, -2.0), np.linspace(1, 3, 5)
    got = Stream(9).s.latin_hypercube(24, 5, lo, hi)
    want = oe.latin_hypercube(oracle.LegacyStream(9), 24, 5, lo, hi)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 127, 128, 129, 135, 255, 256, 1023, 1024, 6143])
def test_sum_plan_reproduces_numpy_pairwise(lib, m):
    """sx_sum_plan drives the kernels' summation order: replay it in Python and compare with ndarray.sum()."""
    buf = np.zeros(4 + 2 * (m // 64 + 2), dtype=np.int32)
    got = lib.sx_sum_plan(m, buf.ctypes.data, buf.size)
    assert got >= 4
    nleaf, tail, mb, depth = (int(v) for v in buf[:4])
    assert mb == m // 8 and tail == (m % 8 if m >= 8 else m)
    a = np.random.RandomState(m).uniform(-1e3, 1e3, m)
    stack, b0 = [], 0
    cur = 0.0
    for t in range(nleaf):
        b1, merges = int(buf[4 + 2 * t]), int(buf[5 + 2 * t])
        r = [a[b0 * 8 + j] for j in range(8)]
        for b in range(b0 + 1, b1):
            for j in range(8):
                r[j] = r[j] + a[b * 8 + j]
        cur = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        if t == nleaf - 1:
            for k in range(tail):
                cur = cur + a[b1 * 8 + k]
        stack.append(cur)
        assert len(stack) <= depth
        for _ in range(merges):
            top = stack.pop()
            stack[-1] = stack[-1] + top
        b0 = b1
    if nleaf == 0:
        for k in range(tail):
            cur = cur + a[k]
        stack = [cur]
    assert len(stack) == 1
    assert 0.0 + stack[0] == a.sum()


def test_row_geometry_numbers_are_pinned(lib):
    """Rows per workgroup and record counts size LDS, grids and the (part_f, part_i) buffers of every row kernel.  The
    expected values restate the sizing rule: a row's LDS budget is n + 8 + 2 (n/64 + 2) doubles above 256 elements and
    3n + 32 + 2 (n/64 + 2) up to there; a workgroup is the largest power-of-two number of waves (<= 8) with <= 16 rows
    and <= 64 KiB of such rows; rows of up to 64 / 128 elements share a wave four / two at a time; beyond the wide
    threshold a workgroup is one row."""
    wide_from = lib.sx_wide_from()
    assert wide_from == 2048

    def rows_per_block(n):
        cap = n // 64 + 2
        stride = n + 8 + 2 * cap if n > 256 else 3 * n + 8 + 24 + 2 * cap
        rpw = 64 // (16 if n <= 64 else 32 if n <= 128 else 64)
        fit = (64 * 1024) // (8 * stride * rpw)
        w = 1
        while 2 * w <= fit and 2 * w * rpw <= 16 and 2 * w <= 8:
            w *= 2
        return w * rpw

    for n in range(1, 4097):
        assert lib.sx_rows_per_workgroup(n) == (1 if n > wide_from else rows_per_block(n)), n
    for P in (2, 37, 4096, 16400):
        for n in (1, 64, 65, 128, 129, 256, 257, 512, 1024, 2048):
            assert lib.sx_num_partials(P, n) == -(-P // rows_per_block(n)), (P, n)


def test_exchange_buffer_geometry(lib):
    """Host side of the peer exchange: slots[2][8][w] + probe[8][w] words of 8 bytes, w = 2(n+2) rounded up to
    whole 128-byte lines; the relay holds two records + their ready lines; bad arguments are refused."""
    for n in (1, 2, 6, 7, 128, 1024, 2560):
        w = -(-2 * (n + 2) // 16) * 16
        assert lib.sx_xchg_bytes(8, n) == 3 * 8 * w * 8 == lib.sx_xchg_bytes(1, n)
        assert lib.sx_xchg_relay_bytes(n) == 2 * (w + 16) * 8
    assert lib.sx_xchg_bytes(9, 8) == -1 and lib.sx_xchg_bytes(0, 8) == -1 and lib.sx_xchg_bytes(2, 0) == -1
    assert lib.sx_xchg_relay_bytes(0) == -1
    from stochopy_amd import _lib

    x = _lib.SxXchgArgs()
    x.world, x.rank = 2, 5  # rank outside the world
    assert lib.sx_xchg_probe(C.byref(x), 8, 1, None) != 0 and b"world / rank" in lib.sx_last_error()


def test_penalize_host_bookkeeping_follows_the_oracle():
    """The host half of constraints="Penalize" (stochopy_amd.optimize._evolution._BoundaryWeights) against the
    oracle's restatement (itself pinned to the reference) over a random walk of the mean in and out of the box:
    identical boundary weights / history / flags, and the same penalised fitness."""
    import oracle
    from oracle import engine as oe
    from stochopy_amd.optimize._evolution import _BoundaryWeights

    rs = np.random.RandomState(5)
    n, P, mueff = 7, 12, 3.4
    ref, got = oe.PenalizeState(n), _BoundaryWeights(n)
    fun = oracle.OBJECTIVES["sphere"]
    xold = np.zeros(n)
    xmean = rs.uniform(-0.5, 0.5, n)
    for it in range(1, 60):
        sigma = 0.05 + 0.3 * rs.rand()
        diagC = rs.uniform(0.2, 3.0, n)
        arx = xmean + sigma * rs.randn(P, n) * np.sqrt(diagC)
        fit_ref, valid = ref.apply(arx, xmean, xold, sigma, diagC, mueff, it, fun)
        raw = fun(np.clip(arx, -1.0, 1.0))
        v = got.update(raw, xmean, xold, sigma, diagC, mueff, it, P)
        assert np.array_equal(got.weights, ref.weights) and np.array_equal(got.spreads, ref.dfithist)
        assert (got.have_spread, got.initial_phase) == (ref.validfitval, ref.iniphase)
        assert np.allclose(raw + ((np.clip(arx, -1.0, 1.0) - arx) ** 2) @ v, fit_ref, rtol=1e-13)
        xold, xmean = xmean, xmean + rs.uniform(-0.4, 0.6, n) * (1.0 if it % 7 else -2.0)
    assert ref.weights.max() > 0.0 and not ref.iniphase  # the walk did leave the box and weights did grow


def test_api_surface_and_validation():
    """Signatures/defaults of the reference (de/_de.py:13-33 etc.) and its bare ValueError/TypeError validation."""
    import inspect

    import stochopy_amd as sa

    sig = inspect.signature(sa.optimize.minimize)
    assert list(sig.parameters) == ["fun", "bounds", "x0", "args", "method", "options", "callback"]
    assert sig.parameters["method"].default == "de"
    de = inspect.signature(sa.optimize.de).parameters
    assert (de["maxiter"].default, de["popsize"].default, de["mutation"].default, de["recombination"].default,
            de["strategy"].default, de["updating"].default, de["xtol"].default) == (100, 10, 0.5, 0.9, "best1bin",
                                                                                    "immediate", 1e-8)
    cp = inspect.signature(sa.optimize.cpso).parameters
    assert (cp["inertia"].default, cp["cognitivity"].default, cp["sociability"].default,
            cp["competitivity"].default) == (0.7298, 1.49618, 1.49618, 1.0)
    assert "competitivity" not in inspect.signature(sa.optimize.pso).parameters
    cm = inspect.signature(sa.optimize.cmaes).parameters
    assert (cm["sigma"].default, cm["muperc"].default) == (0.1, 0.5) and "updating" not in cm
    f, b = sa.factory.rosenbrock, [[-5.12, 5.12]] * 2
    with pytest.raises(TypeError):
        sa.optimize.minimize(42, b)
    # any other Python callable is the reference's fun(x, *args) (SURVEY.md 8b iii): accepted, evaluated per row on
    # the host between the device kernels -- which still needs the GPU (here: the loud no-device error, not a refusal)
    from stochopy_amd._device import NoDeviceError
    from stochopy_amd.optimize import _common

    assert isinstance(_common.resolve_objective(lambda x: float(np.sum(x)), ()), _common.HostExternal)
    # host pools for such an objective: explicit options, or the reference's own spelling (its _common.py:94-97)
    plain = lambda x: float(np.sum(x))  # noqa: E731
    ext = _common.resolve_objective(plain, (), host_workers=3, host_backend="loky")
    assert (ext.pool.workers, ext.pool.backend, ext.from_reference_options) == (3, "loky", False)
    ext = _common.resolve_objective(plain, (), host_workers=2)
    assert ext.pool.backend == "threading"  # the reference's default backend
    ext = _common.resolve_objective(plain, (), workers=5, backend="threading")
    assert (ext.pool.workers, ext.from_reference_options) == (5, True)
    assert _common.resolve_workers(5, ext) == 1 and _common.resolve_backend("threading", ext) == "hip"
    assert _common.resolve_objective(plain, (), workers=1, backend="loky").pool is None  # serial, as in the reference
    assert _common.resolve_objective(plain, (), host_workers=-1).pool.workers == (os.cpu_count() or 1) or (os.cpu_count() or 1) < 2
    with pytest.raises(ValueError):
        _common.resolve_objective(plain, (), host_workers=4, host_backend="mpi")
    with pytest.raises(ValueError):
        _common.resolve_objective(plain, (), workers=4, backend="loky", host_workers=2)
    with pytest.raises(ValueError):  # a factory objective runs in the kernels: no host pool to configure
        _common.resolve_objective(f, (), host_workers=4)
    with pytest.raises(ValueError, match="belongs to keurfonluu/stochopy"):
        sa.optimize.minimize(f, b, options={"backend": "loky", "workers": 4})
    # the pool's tasks are the reference's serial wrapper on blocks of rows
    rows = np.arange(12.0).reshape(4, 3)
    for backend in ("threading", "loky"):
        pool = _common.HostPool(2, backend)
        got = pool.executor().submit(_common._eval_block, np.sum, rows, ()).result()
        assert np.array_equal(got, rows.sum(axis=1))
        pool.close()
    import torch

    host_opts = {"backend": "hip", "updating": "deferred", "maxiter": 3, "popsize": 8, "seed": 0}
    if torch.cuda.is_available():  # (the suite on a GPU box: accepted, and evaluated on the host between the kernels)
        res = sa.optimize.minimize(lambda x: float(np.sum(x)), b, options=host_opts)
        assert 1 <= res.nit <= 3 and res.fun == float(np.sum(res.x))
    else:
        with pytest.raises(NoDeviceError):
            sa.optimize.minimize(lambda x: float(np.sum(x)), b, options=host_opts)
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, [-1, 1])
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, options={"popsize": 1})
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, options={"mutation": 3.0})
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, method="cpso", options={"inertia": 1.5})
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, method="cmaes", options={"sigma": 0.0})
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, options={"backend": "cuda"})
    with pytest.raises(ValueError):
        sa.optimize.minimize(f, b, options={"backend": "loky"})
    with pytest.raises(KeyError):
        sa.optimize.minimize(f, b, method="sampler")  # not an optimizer of the reference's registry


def test_optimize_result_surface():
    """stochopy/_common.py:1-35: dict with attribute access; repr sorted, right-justified, hides xall/funall."""
    from stochopy_amd.optimize import OptimizeResult

    r = OptimizeResult(x=np.array([1.0]), fun=2.0, nit=3, xall=np.zeros(3), funall=np.zeros(3))
    assert r.fun == 2.0 and r["nit"] == 3 and sorted(dir(r)) == ["fun", "funall", "nit", "x", "xall"]
    # width = longest key (incl. the hidden ones) + 1, as in the reference
    assert repr(r).splitlines()[0] == "    fun: 2.0" and "xall" not in repr(r)
    with pytest.raises(AttributeError):
        r.missing
    assert repr(OptimizeResult()) == "OptimizeResult()"


def test_no_gpu_means_loud_failure():
    """Without a ROCm device the product path must raise -- there is no CPU fallback."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import stochopy_amd as sa
    from stochopy_amd._device import NoDeviceError

    with pytest.raises(NoDeviceError):
        sa.optimize.minimize(sa.factory.sphere, [[-1, 1]] * 3, options={"maxiter": 3, "popsize": 8, "seed": 0})
    with pytest.raises(NoDeviceError):
        sa.factory.sphere(np.ones(4))


def test_product_never_imports_the_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "stochopy_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp")):
                text = open(os.path.join(root, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f


def test_workers_option_resolution():
    """`workers` = number of GPUs; None / 0 / 1 = one; -1 = all ranks of the process group (none here -> 1)."""
    from stochopy_amd.optimize import _common

    assert [_common.resolve_workers(w) for w in (None, 0, 1, -1, 4)] == [1, 1, 1, 1, 4]
    with pytest.raises(ValueError):
        _common.resolve_workers(-3)


def test_chained_generations_are_planned_as_few_graph_replays():
    """_DeRun.plan_chain (host logic of the chained DE engine): whole 50-generation graphs, a repeated remainder as one
    graph of exactly that even length, a one-off remainder from the 10-generation graph, single launches for the rest;
    the generations always add up and graphs start at the parity they were built for."""
    from stochopy_amd.optimize._de import _DeRun

    plan = _DeRun.plan_chain
    assert plan(200, 0, {}, 50, 10) == [50] * 4
    assert plan(137, 0, {}, 50, 10) == [50, 50, 10, 10, 10] + [0] * 7  # first request: no new graph for 36
    assert plan(9, 3, {}, 50, 10) == [0] * 9
    seen = {}
    assert plan(20, 5, seen, 50, 10) == [10, 10]      # the driver's --steps 20 --warmup 5: first block ...
    assert plan(20, 25, seen, 50, 10) == [20]         # ... and every later one (odd parity, same length)
    assert plan(20, 45, seen, 50, 10) == [20]
    assert plan(20, 64, seen, 50, 10) == [10, 10]     # the other parity is a different graph: counted on its own
    assert plan(20, 84, seen, 50, 10) == [20]
    assert plan(71, 0, seen, 50, 10) == [50, 20, 0]   # 21 left after the whole graph: the (parity 0, 20) graph exists
    rs = np.random.RandomState(3)
    seen, launches = {}, 0
    for _ in range(300):
        n = int(rs.randint(0, 260))
        p = plan(n, launches, seen, 50, 10)
        assert sum(s if s else 1 for s in p) == n
        at = launches
        for s in p:
            assert s == 0 or (s % 2 == 0 and 10 <= s <= 50)
            at += s if s else 1
        launches += n
    assert all(k[1] % 2 == 0 and 10 < k[1] < 50 for k in seen)


def test_oracle_modules_define_every_name_once():
    """The parity anchor must say one thing: no module under oracle/ defines a top-level name, or a method within a
    class, twice (Python silently keeps the last definition, so a stale copy above it passes every test)."""
    import ast
    import glob
    import os

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
    files = sorted(glob.glob(os.path.join(root, "**", "*.py"), recursive=True))
    assert files
    defs = (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)
    twice = []
    for path in files:
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        scopes = [("", tree.body)] + [(c.name + ".", c.body) for c in ast.walk(tree) if isinstance(c, ast.ClassDef)]
        for prefix, body in scopes:
            seen = {}
            for node in body:
                if isinstance(node, defs):
                    if node.name in seen:
                        twice.append(f"{os.path.relpath(path, root)}: {prefix}{node.name} at lines {seen[node.name]} and {node.lineno}")
                    seen[node.name] = node.lineno
    assert not twice, twice


@pytest.mark.parametrize("P,n", [(2, 3), (7, 5), (100, 70), (513, 2), (4096, 128)])
def test_philox_latin_hypercube_oracle_properties(P, n):
    """The counter-based initial population of the throughput mode (oracle side; the HIP kernel is compared with it bit
    for bit in tests/test_gpu_de.py): it IS a Latin hypercube in the reference's sense (_common.py:109-120) -- every
    column visits every stratum of width (upper - lower) / P exactly once, the jitter fills the LOWER HALF of the cell
    (rand / P inside strata 2 / P wide) -- and any block of rows can be drawn on its own (sharded runs)."""
    import oracle
    from oracle import engine as oe

    s = oracle.PhiloxStream(99)
    lo, up = np.full(n, -5.12), np.linspace(1.0, 5.12, n)
    X = s.lhs_population(P, n, lo, up)
    cell = (X - lo) / (up - lo) * P
    strata = np.floor(cell).astype(int)
    assert all(sorted(strata[:, j]) == list(range(P)) for j in range(n))
    assert (cell - strata < 0.5 + 1e-9).all()
    parts = [s.lhs_population(P, n, lo, up, row0=r0, rows=min(3, P - r0)) for r0 in range(0, P, 3)]
    assert np.array_equal(np.vstack(parts), X)
    assert not np.array_equal(X, oracle.PhiloxStream(100).lhs_population(P, n, lo, up))
    assert np.array_equal(oe.latin_hypercube(oracle.PhiloxStream(99), P, n, lo, up), X)  # what oracle.minimize starts from


def test_replicated_workers_says_so_once_per_method():
    """workers > 1 where a run cannot be sharded (optimize/_common.py replicated_workers): one warning per method, workers -> 1."""
    import warnings

    from stochopy_amd.optimize import _common

    _common._warned_replicated.discard("unit-test")
    with pytest.warns(UserWarning, match="replicated"):
        assert _common.replicated_workers("unit-test", 4, "a reason") == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert _common.replicated_workers("unit-test", 4, "a reason") == 1


@pytest.mark.parametrize("n,P,expected", [
    (512, 1024, "1" + "2" * 39), (20, 48, "1" + "2" * 39),
    (70, 10, "01" + "02" * 19), (130, 24, "01" + "02" * 19),
    (200, 8, "000001" + "000002" * 5 + "0000"), (300, 12, "000001" + "000002" * 5 + "0000"),
    (512, 16, "0000001" + "0000002" * 4 + "00000")])
def test_cmaes_decomposition_schedule(n, P, expected):
    """Which generations decompose C and how (cmaes/_cmaes.py:301; 1 = from the identity, 2 = started from the previous
    eigenvectors, 0 = none): most GPU tests use shapes that decompose in every generation, so the sparse schedules --
    every second, sixth, seventh generation -- are pinned here, as literals."""
    from stochopy_amd.optimize import _cmaes

    c1, cmu = _cmaes._strategy_constants(n, P, 0.5)[5:7]
    eigeneval, got = 0, ""
    for gen in range(1, 41):
        due = _cmaes.decomposition_due(gen, eigeneval, P, c1, cmu, n)
        if due:
            eigeneval = gen * P
        got += str(due)
    assert got == expected


def test_device_resident_loops_look_schedule():
    """When the host reads the state record of a device-resident run: 1, 2, 4, ... generations apart up to a cap (CMA-ES:
    16, 4, 2, 1 for n = 32, 128, 256, 512; VD-CMA: 16), every generation with a callback or in a sharded run, and always
    after the last generation."""
    from stochopy_amd.optimize import _cmaes, _evolution, _vdcma

    LOOK = _cmaes._CmaDeviceRun.LOOK
    assert [_cmaes.look_cap(n, LOOK) for n in (32, 128, 256, 512)] == [16, 4, 2, 1]
    assert _evolution.look_generations(70, 16, False) == [1, 3, 7, 15, 31, 47, 63, 70]
    assert _evolution.look_generations(70, 4, False) == [1, 3, 7] + list(range(11, 68, 4)) + [70]
    assert _evolution.look_generations(70, 2, False) == list(range(1, 70, 2)) + [70]
    assert _evolution.look_generations(70, 1, False) == list(range(1, 71))
    for cap in (16, 4, 2, 1):  # a callback, a world
        assert _evolution.look_generations(9, cap, True) == list(range(1, 10))
    run = _vdcma._VdDeviceRun.__new__(_vdcma._VdDeviceRun)
    assert run._look_cap() == 16
    assert _evolution.look_generations(100, 16, False) == [1, 3, 7, 15, 31, 47, 63, 79, 95, 100]
    assert _evolution.look_generations(15, 16, False) == [1, 3, 7, 15] and _evolution.look_generations(0, 16, False) == []


def test_cmaes_sweep_allowance_after_a_look():
    """Sweeps launched for the next warm-started decomposition, from the eigensolver's record at a look: what the last one
    used + 1 while the host looks at every generation, + 3 between rarer looks, never more than 60; a short-fall sets it
    to 60 and warns -- "60 sweeps" when 60 had been launched, "ran out of its %d launched sweeps" the first time
    otherwise, nothing later."""
    from stochopy_amd.optimize._cmaes import sweep_allowance

    # (used, ok, fails, fails_seen, launched, look_cap, warned_short)
    assert sweep_allowance(11, True, 0, 0, 16, 1, False) == (12, 0, None)
    assert sweep_allowance(11, True, 0, 0, 16, 4, False) == (14, 0, None)
    assert sweep_allowance(60, True, 2, 2, 60, 1, True) == (60, 2, None)
    assert sweep_allowance(59, True, 0, 0, 60, 16, False) == (60, 0, None)
    sweeps, seen, warning = sweep_allowance(60, False, 1, 0, 60, 1, False)
    assert (sweeps, seen) == (60, 1) and "did not reach its tolerance in 60 sweeps" in warning
    sweeps, seen, warning = sweep_allowance(11, False, 1, 0, 11, 1, False)
    assert (sweeps, seen) == (60, 1) and "ran out of its 11 launched sweeps" in warning
    assert sweep_allowance(12, False, 2, 1, 12, 1, True) == (60, 2, None)
    # a converged record next to a short-fall the host has not seen yet (between rarer looks) is a short-fall
    sweeps, seen, warning = sweep_allowance(9, True, 3, 2, 13, 4, False)
    assert (sweeps, seen) == (60, 3) and "ran out of its 13 launched sweeps" in warning
    assert "60 sweeps" in sweep_allowance(60, True, 3, 2, 60, 4, True)[2]


@pytest.mark.parametrize("module,cls,how,gathered", [("_cmaes", "_CmaDeviceRun", (2,), ["arx", "fit"]),
                                                     ("_vdcma", "_VdDeviceRun", (), ["ary", "arx", "fit"])])
def test_sharded_generation_enqueue_order(module, cls, how, gathered):
    """One sharded generation through the shared enqueue (_DeviceRun._generation): stage 0 on this rank's rows, the gathers
    in the method's order, stage 1; one call on one GPU."""
    import importlib
    import types

    Run = getattr(importlib.import_module("stochopy_amd.optimize." + module), cls)
    events = []
    run = Run.__new__(Run)  # the host logic only: the library calls are stand-ins
    entry, stage = Run.ENTRY, Run.ENTRY + "_stage"

    def record(name):
        return lambda a, *args: events.append((name,) + tuple(getattr(x, "value", x) for x in args)) or 0

    run.ctx = types.SimpleNamespace(L=types.SimpleNamespace(**{entry: record(entry), stage: record(stage)}), stream_ptr="s")
    run.args = Run.Args()
    run.buffers = {k: "full " + k for k in gathered}
    run._local = [types.SimpleNamespace(data_ptr=lambda k=k: 1000 + len(k)) for k in gathered]
    run.world = types.SimpleNamespace(all_gather_rows=lambda loc, full: events.append(("gather", run._local.index(loc), full)))
    run.row0, run.Pl = 24, 8
    run._generation(5, *how)
    assert events == ([(stage, 5, *how, 0, 24, 8, *(1000 + len(k) for k in gathered), "s")]
                      + [("gather", i, "full " + k) for i, k in enumerate(gathered)]
                      + [(stage, 5, *how, 1, 0, 0, *(None for _ in gathered), "s")])
    del events[:]
    run.world = None
    run._generation(6, *how)
    assert events == [(entry, 6, *how, "s")]
