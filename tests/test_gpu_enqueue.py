"""Eager launches against hipGraph nodes, through the C ABI: every generation that can be replayed from a graph is enqueued
by ONE function (csrc/sx_enqueue.hpp) for both sinks, and a run is a mix of replays and an eager tail.  From identical copies
of the initial buffers each case makes K eager calls, and builds a graph of K generations and launches it once; every buffer
the kernels write must then agree BIT FOR BIT (the raw int64 view: NaN payloads and the sign of zero count).

Shapes are the smallest that reach each branch of the host-side dispatch: the compile-time and run-time row lengths, one
batch, the wide generation kernels (n > 2048) with the narrow and the three-kernel best / termination step (n > 4096), the
chained DE kernel from either parity, plain / Shrink / wide PSO, and CPSO as four launches per generation, as two (fused
radius) and on wide rows -- with a restart due in every generation (delta = 1e300, nw between 1 and P - 1).  The
peer-exchange kernel needs ranks: tests/test_distributed.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 3
I64_MAX = np.iinfo(np.int64).max
LO, HI = -5.12, 5.12


@pytest.fixture(scope="module")
def env():
    from stochopy_amd import _device, _lib, _rng

    return _device.Context(), _device, _lib, _rng


def _bits(tensor):
    return tensor.cpu().numpy().reshape(-1).view(np.int64)


def _state_words(_lib, **kw):
    st = _lib.SxState(dx=0.0, status=_lib.SX_STATUS_NONE, done=0, **kw)
    return np.frombuffer(bytes(st), dtype=np.int64).copy()


def _assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for name in want:
        assert np.array_equal(got[name], want[name]), f"{tag}: buffer {name} differs between the eager and the graph form"


def _launch_graph(env, g):
    ctx, _, _lib, _ = env
    try:
        _lib.check(ctx.L.sx_graph_launch(g, ctx.stream_ptr), "sx_graph_launch")
        ctx.sync()
    finally:
        ctx.L.sx_graph_destroy(g)


# ------------------------------------------------------------------------------------------------------------------- DE
def _de_initial(env, n, P, objective, seed):
    """Host copies of a run's initial buffers (generation 1 in buf1, its fitness from the device's own objective)."""
    ctx, _device, _lib, _ = env
    X = np.random.RandomState(seed).uniform(LO, HI, (P, n))
    with _device.torch().cuda.stream(ctx.stream):
        fit = _device.evaluate(ctx, _lib.FUN_IDS[objective], ctx.upload(X), n).cpu().numpy()
    return {"X": X, "fit": fit, "g": int(np.argmin(fit))}


class _DeRun:
    """Fresh device buffers from the initial host copies, and the sx_de_args that point at them."""

    def __init__(self, env, init, n, P, objective, strategy, constraints, chain, seed):
        ctx, _device, _lib, _rng = env
        t = _device.torch()
        self.env, self.chain = env, chain
        g, gfit = init["g"], float(init["fit"][init["g"]])
        npart = int(ctx.L.sx_de_num_partials(P, n, 0))
        with t.cuda.stream(ctx.stream):
            b = self.buf = {"buf0": ctx.zeros((P, n)), "buf1": ctx.upload(init["X"]), "fit": ctx.upload(init["fit"]),
                            "candfit": ctx.upload(init["fit"])}
            self.bounds = ctx.upload(np.concatenate([np.full(n, LO), np.full(n, HI)]))
            if chain:  # state[3] + records[2][npart]: launch 0 (parity 0) first "finalises" generation 1 from records[0]
                pf, pi = np.full((2, npart), np.inf), np.full((2, npart), I64_MAX, dtype=np.int64)
                pf[0, 0], pi[0, 0] = gfit, g
                b["part_f"], b["part_i"] = ctx.upload(pf), ctx.upload(pi)
                st = _state_words(_lib, it=1, gbidx=g, gfit=gfit)
                b["state"] = ctx.upload(np.concatenate([_state_words(_lib, it=0, gbidx=g, gfit=gfit), st, st]))
            else:
                b["part_f"], b["part_i"] = ctx.zeros((npart,)), ctx.zeros((npart,), dtype=t.int64)
                b["state"] = ctx.upload(_state_words(_lib, it=1, gbidx=g, gfit=gfit))
                b["gbest"] = ctx.upload(init["X"][g])
        a = self.args = _lib.SxDeArgs()
        a.buf0, a.buf1, a.fit, a.candfit = (b[k].data_ptr() for k in ("buf0", "buf1", "fit", "candfit"))
        a.lower, a.upper = self.bounds[:n].data_ptr(), self.bounds[n:].data_ptr()
        a.state, a.part_f, a.part_i = b["state"].data_ptr(), b["part_f"].data_ptr(), b["part_i"].data_ptr()
        a.gbest = None if chain else b["gbest"].data_ptr()
        a.P, a.ld, a.row0, a.n, a.wide_from = P, n, 0, n, 0
        a.fun_id, a.strategy = _lib.FUN_IDS[objective], _lib.DE_STRATEGIES[strategy]
        a.constraints, a.rng, a.maxiter = (1 if constraints == "Random" else 0), _lib.SX_RNG_PHILOX, 1000
        a.F, a.CR, a.xtol, a.ftol = 0.5, 0.9, 1e-8, 1e-8
        a.key0, a.key1 = _rng.philox_key(seed)

    def generations(self, k):
        ctx, _, _lib, _ = self.env
        for _ in range(k):
            _lib.check(ctx.L.sx_de_generation(C.byref(self.args), 1, ctx.stream_ptr), "sx_de_generation")

    def graph(self, k):
        ctx, _, _lib, _ = self.env
        g = C.c_void_p()
        _lib.check(ctx.L.sx_de_graph_create(C.byref(self.args), k, C.byref(g)), "sx_de_graph_create")
        _launch_graph(self.env, g)

    def chain_launch(self, parity, finalize_only=0):
        ctx, _, _lib, _ = self.env
        _lib.check(ctx.L.sx_de_chain_launch(C.byref(self.args), parity, finalize_only, ctx.stream_ptr), "sx_de_chain_launch")

    def chain_graph(self, k, start_parity):
        ctx, _, _lib, _ = self.env
        g = C.c_void_p()
        _lib.check(ctx.L.sx_de_chain_graph_create(C.byref(self.args), k, start_parity, C.byref(g)),
                   "sx_de_chain_graph_create")
        _launch_graph(self.env, g)

    def read(self):
        self.env[0].sync()
        return {k: _bits(v) for k, v in self.buf.items()}


DE_CASES = [  # n, P, strategy, constraints
    (5, 8, "best1bin", None),
    (5, 8, "rand2bin", "Random"),
    (128, 64, "best1bin", None),  # compile-time row length
    (200, 16, "best1bin", None),  # one batch, run-time length
    (2049, 8, "best1bin", None),  # wide generation, narrow best / termination
    (4097, 8, "best1bin", None),  # wide generation, three-kernel best / termination
]


@pytest.mark.parametrize("n,P,strategy,constraints", DE_CASES)
def test_de_graph_of_generations_equals_eager_generations(env, n, P, strategy, constraints):
    init = _de_initial(env, n, P, "rastrigin", seed=n + P)
    mk = lambda: _DeRun(env, init, n, P, "rastrigin", strategy, constraints, chain=False, seed=1000 + n)  # noqa: E731
    eager, graph = mk(), mk()
    eager.generations(K)
    want = eager.read()
    graph.graph(K)
    got = graph.read()
    assert int(want["state"][0]) == 1 + K  # (the generations did run)
    assert not np.array_equal(want["buf0"], _bits(eager.env[0].zeros((P, n))))
    _assert_same(got, want, (n, P, strategy, constraints))


@pytest.mark.parametrize("n,P", [(128, 64), (5, 8)])
def test_de_chained_graph_equals_eager_launches_from_either_parity(env, n, P):
    init = _de_initial(env, n, P, "rastrigin", seed=n + P)
    mk = lambda: _DeRun(env, init, n, P, "rastrigin", "best1bin", None, chain=True, seed=2000 + n)  # noqa: E731
    eager, graph, mixed = mk(), mk(), mk()
    for parity in (0, 1, 0, 1):
        eager.chain_launch(parity)
    eager.chain_launch(0, finalize_only=1)
    want = eager.read()
    assert int(want["state"][2 * 8]) == 1 + 4  # state[2].it: four generations behind the initial one, finalised
    graph.chain_graph(4, 0)
    graph.chain_launch(0, finalize_only=1)
    _assert_same(graph.read(), want, (n, P, "graph of 4 from parity 0"))
    mixed.chain_launch(0)
    mixed.chain_graph(3, 1)
    mixed.chain_launch(0, finalize_only=1)
    _assert_same(mixed.read(), want, (n, P, "one eager launch, then a graph of 3 from parity 1"))


# ------------------------------------------------------------------------------------------------------------ PSO / CPSO
DELTA, GAMMA = 1e300, 1.0


class _PsoRun:
    def __init__(self, env, init, n, P, objective, shrink, it0, seed):
        ctx, _device, _lib, _rng = env
        t = _device.torch()
        self.env = env
        g, gfit = init["g"], float(init["fit"][init["g"]])
        npart = int(ctx.L.sx_num_partials(P, n))
        with t.cuda.stream(ctx.stream):
            b = self.buf = {"X": ctx.upload(init["X"]), "V": ctx.zeros((P, n)), "pbest": ctx.upload(init["X"]),
                            "pbestfit": ctx.upload(init["fit"]), "gbest": ctx.upload(init["X"][g]),
                            "state": ctx.upload(_state_words(_lib, it=it0, gbidx=g, gfit=gfit)),
                            "sel3": ctx.zeros((3,), dtype=t.int64)}
            self.candfit = ctx.upload(init["fit"])
            self.part_f, self.part_i = ctx.zeros((npart,)), ctx.zeros((npart,), dtype=t.int64)
            self.part_r = ctx.zeros((npart,))
            self.bounds = ctx.upload(np.concatenate([np.full(n, LO), np.full(n, HI)]))
        a = self.args = _lib.SxPsoArgs()
        a.X, a.V, a.pbest, a.pbestfit, a.gbest = (b[k].data_ptr() for k in ("X", "V", "pbest", "pbestfit", "gbest"))
        a.candfit, a.state = self.candfit.data_ptr(), b["state"].data_ptr()
        a.lower, a.upper = self.bounds[:n].data_ptr(), self.bounds[n:].data_ptr()
        a.part_f, a.part_i = self.part_f.data_ptr(), self.part_i.data_ptr()
        a.P, a.ld, a.row0, a.n, a.fun_id = P, n, 0, n, _lib.FUN_IDS[objective]
        a.constraints, a.rng, a.maxiter = (1 if shrink else 0), _lib.SX_RNG_PHILOX, 1000
        a.w, a.c1, a.c2, a.xtol, a.ftol = 0.7298, 1.49618, 1.49618, 1e-8, 1e-8
        a.key0, a.key1 = _rng.philox_key(seed)

    def generations(self, k, restart):
        ctx, _device, _lib, _ = self.env
        a, p, sp = C.byref(self.args), _device.ptr, ctx.stream_ptr
        for _ in range(k):
            _lib.check(ctx.L.sx_pso_generation(a, 1, sp), "sx_pso_generation")
            if restart:
                _lib.check(ctx.L.sx_pso_radius(a, p(self.part_r), sp), "sx_pso_radius")
                _lib.check(ctx.L.sx_pso_restart_select(a, p(self.part_r), DELTA, GAMMA, p(self.buf["sel3"]), sp),
                           "sx_pso_restart_select")
                _lib.check(ctx.L.sx_pso_restart_apply(a, p(self.buf["sel3"]), None, None, 0, sp), "sx_pso_restart_apply")

    def graph(self, k, restart):
        ctx, _device, _lib, _ = self.env
        g, p = C.c_void_p(), _device.ptr
        _lib.check(ctx.L.sx_pso_graph_create(C.byref(self.args), k, p(self.part_r) if restart else None,
                                             DELTA if restart else 0.0, GAMMA if restart else 0.0,
                                             p(self.buf["sel3"]) if restart else None, C.byref(g)), "sx_pso_graph_create")
        _launch_graph(self.env, g)

    def read(self):
        self.env[0].sync()
        return {k: _bits(v) for k, v in self.buf.items()}


def _pso_pair(env, n, P, shrink, restart):
    init = _de_initial(env, n, P, "rastrigin", seed=3 * n + P)
    it0 = 400 if restart else 1
    mk = lambda: _PsoRun(env, init, n, P, "rastrigin", shrink, it0, seed=3000 + n)  # noqa: E731
    eager, graph = mk(), mk()
    eager.generations(K, restart)
    want = eager.read()
    graph.graph(K, restart)
    assert int(want["state"][0]) == it0 + K
    return graph.read(), want


@pytest.mark.parametrize("n,P,shrink", [(64, 32, False), (10, 8, True), (2049, 4, False)])
def test_pso_graph_of_generations_equals_eager_generations(env, n, P, shrink):
    got, want = _pso_pair(env, n, P, shrink, restart=False)
    _assert_same(got, want, (n, P, shrink))


@pytest.mark.parametrize("n,P,form", [(10, 16, "four"), (64, 32, "fused"), (64, 32, "fused-exact"), (4097, 4, "four")])
def test_cpso_graph_with_restarts_equals_the_four_eager_launches(env, n, P, form, monkeypatch):
    """(10, 16): four launches per generation in the graph too; (64, 32): two, the radius a by-product of the generation
    kernel; (4097, 4): the wide kernels.  gamma = 1 at generations 401 ... 403 of 1000 and delta = 1e300: every generation
    decides a restart of nw rows, 1 <= nw <= P - 1, which the graph carries out inside the next generation kernel (and
    behind the last one), the eager sequence by a launch of its own.

    sel3 is {nw, threshold key, radius}.  The two-launch form settles `radius < delta` from the radius against the PREVIOUS
    best and the step of the best wherever that suffices (cpso_post_kernel, csrc/sx_pso.hip), and then leaves THAT radius
    in word 2 -- nothing reads it -- where the eager radius kernel measures against the new best: measured at (64, 32),
    generation 403, the graph leaves 0x3ff695978470633b and the eager sequence 0x3ffef78ccde3a0ed, on the build before the
    shared enqueue path as on the one with it.
    So "fused" compares words 0 and 1 of sel3 and every other buffer, and "fused-exact" sends every generation through the
    kernel's exact branch (SX_CPSO_FORCE_EXACT=1, read when the graph is created), whose radius word must agree too."""
    if form == "fused-exact":
        monkeypatch.setenv("SX_CPSO_FORCE_EXACT", "1")
    got, want = _pso_pair(env, n, P, False, restart=True)
    nw = int(want["sel3"][0])
    assert 1 <= nw <= P - 1, nw
    assert np.count_nonzero(want["pbestfit"].view(np.float64) == 1.0e30) >= nw  # (the last restart's rows, re-seeded)
    if form == "fused":
        got["sel3"], want["sel3"] = got["sel3"][:2], want["sel3"][:2]
    _assert_same(got, want, (n, P, form))
