"""The single-GPU chained DE kernel stores a row of up to 128 elements BEFORE the objective and again after it
(csrc/sx_de_kernel.hpp SX_SPEC_*, sx_de_args.spec_store: 0 = the trial early and the winner late, which is what runs;
1 = once, late; 2 / 3 = the trial / the old row early and afterwards only the rows for which that was the wrong one).
Whatever the mode, every generation's population is the oracle's, bit for bit.

The modes act on rows of up to 128 elements; the whole-wave forms -- the n = 256 and n = 200 cases -- store late whatever
spec_store says, and must give the same bits too.  No output bit depends on the mode, so no test can see which stores a
launch made: that modes 2 and 3 store rows a second time in these runs rests on the oracle's win fractions asserted below.

Every case drives `_DeRun` through the chained path (Philox draws, no callback on the device side) and compares with
`oracle.minimize(..., rng="philox", updating="deferred")`, whose callback hands out every generation's population."""
import functools

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

GENS = 60
SEED = 7
BOUND = 5.12
F, CR = 0.55, 0.9  # (with the headline's F = 0.5 the n = 64 run has a single generation with few winners)
MODES = [0, 1, 2, 3]  # 0 = trial early + winner late, 1 = late, 2 = trial-early, 3 = old-early
# the smallest shapes that reach each one-batch kernel form with more than one workgroup
SHAPES = [
    (64, 64),    # compile-time row length, 16 lanes per row: 4 workgroups of 16 rows
    (128, 32),   # compile-time row length, 32 lanes per row: 2 workgroups of 16 rows
    (256, 16),   # compile-time row length, 64 lanes per row: 2 workgroups of 8 rows
    (100, 40),   # general short row: lanes past the row's end, 3 workgroups, the last with 8 inactive rows
    (200, 24),   # whole-wave one-batch row of run-time length (ONEB): 3 workgroups of 8 rows
]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


@functools.lru_cache(maxsize=None)
def reference(objective, n, P, strategy, ftol=-1.0, maxiter=GENS):
    """The oracle's run, computed once per configuration and shared (read-only) by the cases that need it: the result,
    every generation's population, and the fraction of rows each generation replaced."""
    pops = []
    opts = {"maxiter": maxiter, "popsize": P, "seed": SEED, "strategy": strategy, "updating": "deferred", "ftol": ftol,
            "xtol": 0.0, "mutation": F, "recombination": CR}
    res = oracle.minimize(objective, [[-BOUND, BOUND]] * n, method="de", options=opts, rng="philox",
                          callback=lambda X, r: pops.append(X.copy()))
    for X in pops:
        X.setflags(write=False)
    wins = [float(np.any(a != b, axis=1).mean()) for a, b in zip(pops, pops[1:])]
    return res, pops, wins


def make_run(sa, objective, n, P, strategy, spec_store, ftol=-1.0, maxiter=GENS):
    from stochopy_amd import _lib
    from stochopy_amd.optimize import _de

    run = _de._DeRun(_lib.FUN_IDS[objective], np.full(n, -BOUND), np.full(n, BOUND), None, maxiter, P, F, CR, strategy, None,
                     0.0, ftol, False, 1.0, None, "philox", SEED, 1, autorun=False, spec_store=spec_store)
    assert run.chain, "the case must take the chained kernel"
    return run


def stepwise_populations(run, gens):
    """Generation 1 and the `gens - 1` after it, one eager launch each: [(state, population)]."""
    import torch

    out = []
    with torch.cuda.stream(run.ctx.stream):
        run._setup()
        st = run.read_state()
        out.append((st, run._population(st.it).cpu().numpy()))
        for _ in range(gens - 1):
            run.enqueue(1)
            st = run.read_state()
            out.append((st, run._population(st.it).cpu().numpy()))
    return out


def check_against_oracle(sa, objective, n, P, strategy, spec_store):
    res, pops, _ = reference(objective, n, P, strategy)
    assert len(pops) == GENS
    run = make_run(sa, objective, n, P, strategy, spec_store)
    try:
        got = stepwise_populations(run, GENS)
        last = got[-1][0]
        x = run._best_row(last)
    finally:
        run.close()
    for g, ((st, X), Xref) in enumerate(zip(got, pops), start=1):
        assert int(st.it) == g
        assert 0 <= int(st.gbidx) < P
        assert np.array_equal(X, Xref), "generation %d: %d rows differ" % (g, int(np.any(X != Xref, axis=1).sum()))
    assert int(last.it) == res.nit == GENS and float(last.gfit) == float(res.fun) and np.array_equal(x, res.x)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_p%d" % s)
def test_best1bin_oracle_runs_visit_every_win_fraction(shape):
    """What makes the cases below reach both branches of every store mode (rows stored again, rows left alone), asserted on
    the oracle's own trajectory: the run starts with few winners, passes through about one half, and then most rows win
    for most of the run."""
    n, P = shape
    wins = reference("rosenbrock", n, P, "best1bin")[2]
    assert len(wins) == GENS - 1
    assert sum(w <= 0.25 for w in wins) >= 2, wins
    assert sum(0.4 <= w <= 0.6 for w in wins) >= 1, wins
    assert sum(w >= 0.75 for w in wins) >= 10, wins


def test_rand1bin_oracle_run_keeps_losing():
    """rand1bin at n = 128, P = 32: at most a quarter of the rows win in any generation, so under trial-early nearly
    every row is stored a second time."""
    wins = reference("sphere", 128, 32, "rand1bin")[2]
    assert max(wins) <= 0.25, wins


@pytest.mark.parametrize("spec_store", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_p%d" % s)
def test_every_generation_matches_oracle(sa, shape, spec_store):
    n, P = shape
    check_against_oracle(sa, "rosenbrock", n, P, "best1bin", spec_store)


@pytest.mark.parametrize("spec_store", MODES)
def test_rand1bin_mostly_losing_rows_match_oracle(sa, spec_store):
    check_against_oracle(sa, "sphere", 128, 32, "rand1bin", spec_store)


@pytest.mark.parametrize("spec_store", MODES)
def test_graph_replay_equals_eager_launches(sa, spec_store):
    """60 launches as enqueue(50) + enqueue(10) (two replayed graphs) and as sixty eager ones: the same bits, and the
    oracle's.  maxiter = 60 stops the run in the last launch, which must leave the other buffer alone."""
    import torch

    n, P = 128, 32
    res, pops, _ = reference("rosenbrock", n, P, "best1bin")
    got = []
    for plan in ([50, 10], [1] * 60):
        run = make_run(sa, "rosenbrock", n, P, "best1bin", spec_store)
        try:
            with torch.cuda.stream(run.ctx.stream):
                run._setup()
                for k in plan:
                    run.enqueue(k)
                st = run.read_state()
                got.append((int(st.it), float(st.gfit), int(st.gbidx), run._population(st.it).cpu().numpy(),
                            run._population(st.it - 1).cpu().numpy(), run.fit.cpu().numpy()))
        finally:
            run.close()
    a, b = got
    assert a[:3] == b[:3] and a[0] == res.nit == GENS and a[1] == float(res.fun)
    for u, v in zip(a[3:], b[3:]):
        assert np.array_equal(u, v)
    assert np.array_equal(a[3], pops[GENS - 1]) and np.array_equal(a[4], pops[GENS - 2])


@functools.lru_cache(maxsize=None)
def ftol_reference(n, P):
    """An ftol the free run meets at generation 30 or before (its best value there; best values only fall), and the
    oracle's run under it."""
    free, pops, _ = reference("rosenbrock", n, P, "best1bin")
    ftol = float(oracle.OBJECTIVES["rosenbrock"](pops[29]).min())
    assert ftol > float(free.fun)
    res, stopped, _ = reference("rosenbrock", n, P, "best1bin", ftol=ftol)
    assert 2 <= res.nit <= 30 and len(stopped) == res.nit and res.status >= 0
    return ftol, res, stopped


@pytest.mark.parametrize("spec_store", MODES)
def test_ftol_stop_inside_a_graph_stores_nothing_more(sa, spec_store):
    """An ftol that the run meets inside a 50-generation graph: the launches behind the stop are no-ops and must not store a
    row, early or late.  x, fun, nit and the final population are the oracle's."""
    import torch

    n, P = 128, 32
    ftol, res, pops = ftol_reference(n, P)
    run = make_run(sa, "rosenbrock", n, P, "best1bin", spec_store, ftol=ftol)
    try:
        with torch.cuda.stream(run.ctx.stream):
            run._setup()
            run.enqueue(50)
            st = run.read_state()
            X = run._population(st.it).cpu().numpy()
            Xprev = run._population(st.it - 1).cpu().numpy()
            x = run._best_row(st)
    finally:
        run.close()
    assert int(st.it) == res.nit and bool(st.done) and float(st.gfit) == float(res.fun)
    assert np.array_equal(x, res.x)
    assert np.array_equal(X, pops[-1])
    assert np.array_equal(Xprev, pops[-2])  # the other buffer: what a launch behind the stop would have written over


@pytest.mark.parametrize("spec_store", MODES)
def test_finalise_reports_a_plain_row(sa, spec_store):
    """What the host reads after a run is a row index below P."""
    import torch

    n, P = 128, 32
    res, pops, _ = reference("rosenbrock", n, P, "best1bin")
    run = make_run(sa, "rosenbrock", n, P, "best1bin", spec_store)
    try:
        with torch.cuda.stream(run.ctx.stream):
            run._setup()
            run.enqueue(GENS - 1)
            st = run.read_state()
            X = run._population(st.it).cpu().numpy()
    finally:
        run.close()
    assert int(st.it) == GENS
    assert 0 <= int(st.gbidx) < P and 0 <= int(st.reserved[0]) < P
    assert np.array_equal(X[int(st.gbidx)], res.x) and float(st.gfit) == float(res.fun)
