"""The deferred (updating="deferred") DE and PSO / CPSO generation kernels for the tests: the table of whole runs that
tests/test_gpu_deferred_forms.py holds against the oracle bit for bit (and tests/test_deferred_cases_host.py checks on the
oracle alone), the oracle run every comparison shares, and the drivers of the launch forms.  A plain helper module (imported,
not collected); nothing here touches the device at import.

The oracle is handed a callable that returns the DEVICE's values (`stochopy_amd.factory.<name>(X)`: sx_eval).  A row's
objective value is the same bits in every kernel, so the oracle's proposals, selections and stops are then the fused run's
for all seven objectives: every comparison is `np.array_equal` / `==`.

Which kernel a case reaches is decided by `pick_kernel` (csrc/sx_de_kernel.hpp, csrc/sx_pso.hip); `de_form` / `pso_form`
below restate those dispatchers, so that the host test can count the forms the table visits.  The forms:

  DE, chained kernel (XM = 1: Philox draws, no callback -- what `_DeRun.enqueue` launches) and two-kernel path (XM = 0:
  `minimize(..., callback=...)`, and every run with host draws), 16 / 32 / 64 lanes per row for n <= 64 / <= 128 / larger:
    general      run-time row length, strategy and constraints (every non-hot objective, rand2bin / best2bin, Random,
                 host draws);
    STRAT        run-time row length, strategy at compile time (hot objective, best1bin / rand1bin, constraints=None);
    ONEB         STRAT for whole-wave rows of up to 256 elements: one batch;
    FULL         chained only: whole workgroups and n a multiple of 4 * lanes: no bounds test (non-hot objectives at
                 n = 64 / 128 / 256, every objective at n = 512 / 1024 -- where the summation plan is a compile-time one);
    NFIX         FULL with n = 4 * lanes as a compile-time constant (hot objectives; rand2bin / best2bin or Random);
    NFIX+STRAT   NFIX with best1bin / rand1bin and constraints=None.
  PSO / CPSO:
    general      everything else;   PLAIN  hot objective, constraints=None, no restart pending;
    FULL         n = 64 / 128 / 256 with Philox draws (compile-time row length); FULL+PLAIN likewise;
    FULL+RAD     FULL inside a replayed CPSO graph: the swarm radius as a by-product;
    ONEB, ONEB+PLAIN   hot objective, whole-wave rows of run-time length up to 256 (n = 130, 200).
"""
import collections
import contextlib
import functools
import zlib

import numpy as np

import oracle
from oracle import engine
from oracle.objectives import OBJECTIVES

ALL = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")
HOT = ("ackley", "rastrigin", "rosenbrock", "sphere")       # csrc/sx_device.hpp hot_objective
COLD = ("griewank", "quartic", "styblinski_tang")
INEXACT = ("ackley", "griewank", "rastrigin")                # cos / exp / sqrt: the device's last bits are not numpy's
STRATEGIES = ("rand1bin", "best1bin", "rand2bin", "best2bin")
SPECIAL_STRATEGIES = ("best1bin", "rand1bin")                # the two with compile-time forms
BOUND = 5.12
GENS = 8          # a case is a whole run of this many generations
GRAPH_GENS = 23   # DE: two replays of the 10-generation graph and three eager launches; PSO: one 16-generation graph and seven
STOP_GEN = 4      # a stop case ends here
NS = (3, 17, 64, 100, 128, 130, 200, 256, 300)
HOST_NS = (17, 100, 200)  # of the sweeps' row lengths, the ones run on host draws: one per lanes-per-row class

RANDOM = {"constraints": "Random", "mutation": 1.5}                                          # repairs happen
SHRINK = {"constraints": "Shrink", "inertia": 1.0, "cognitivity": 3.0, "sociability": 3.0}  # particles do leave the box

# tag, method, objective, n, pop ("whole": two whole workgroups; "ragged": two and three rows; or a number), rng, the
# method's own options, kind ("run", or "stop1" / "stop0": ends at STOP_GEN with that status), graph (also run as one
# minimize() of GRAPH_GENS generations without a callback), restart (cpso: restarts fire)
Case = collections.namedtuple("Case", "tag method objective n pop rng options kind graph restart seed")


def lanes_per_row(n):
    return 16 if n <= 64 else (32 if n <= 128 else 64)


@functools.lru_cache(maxsize=None)
def rows_per_workgroup(n):
    from stochopy_amd import _lib

    return int(_lib.lib().sx_rows_per_workgroup(n))


def popsize(case):
    if case.pop == "whole":
        return 2 * rows_per_workgroup(case.n)
    if case.pop == "ragged":
        return 2 * rows_per_workgroup(case.n) + 3
    return int(case.pop)


def seed_of(case):
    """The case's own seed where the table names one (a stop case needs a run whose best value falls AT generation
    STOP_GEN), else one derived from its tag."""
    return case.seed if case.seed is not None else 1 + zlib.crc32(case.tag.encode()) % 997


def bounds(case):
    return [[-BOUND, BOUND]] * case.n


def run_options(case, maxiter=GENS, ftol=-1.0, xtol=0.0):
    """The options of the case's run, as both `oracle.minimize` and `stochopy_amd.optimize.minimize` take them."""
    return dict(case.options, maxiter=maxiter, popsize=popsize(case), seed=seed_of(case), updating="deferred", ftol=ftol,
                xtol=xtol)


# ---- the dispatchers, restated ------------------------------------------------------------------------------------------
def de_form(case, chained):
    """The branch of `pick_kernel` (csrc/sx_de_kernel.hpp) the case's generation kernel comes from: (form, lanes per row)."""
    n, P, lpr = case.n, popsize(case), lanes_per_row(case.n)
    hot, philox = case.objective in HOT, case.rng == "philox"
    special = case.options.get("constraints") is None and case.options["strategy"] in SPECIAL_STRATEGIES
    assert philox or not chained
    full = chained and n % (4 * lpr) == 0 and P % rows_per_workgroup(n) == 0
    if full and philox and n == 4 * lpr and hot:
        return ("NFIX+STRAT" if special else "NFIX"), lpr
    if full:
        return "FULL", lpr
    if philox and hot and special:
        return ("ONEB" if lpr == 64 and n <= 256 else "STRAT"), lpr
    return "general", lpr


def pso_form(case, in_graph=False):
    """The branch of `pick_kernel` (csrc/sx_pso.hip): (form, lanes per row).  `in_graph`: the generations a replayed graph
    holds -- with cpso they carry the restart (never PLAIN), and whole-batch rows leave the radius by-product."""
    n, lpr = case.n, lanes_per_row(case.n)
    hot, philox = case.objective in HOT, case.rng == "philox"
    carries_restart = in_graph and case.method == "cpso"
    plain = case.options.get("constraints") is None and not carries_restart and hot and philox
    if philox and n == 4 * lpr:
        return ("FULL+PLAIN" if plain else "FULL+RAD" if carries_restart else "FULL"), lpr
    if philox and lpr == 64 and n <= 256 and hot:
        return ("ONEB+PLAIN" if plain else "ONEB"), lpr
    return ("PLAIN" if plain else "general"), lpr


def forms(case):
    """Every (method family, form, lanes per row, draws) the case's launch forms reach."""
    out = set()
    if case.method == "de":
        out.add(("de-two-kernel", *de_form(case, False), case.rng))
        if case.rng == "philox":
            out.add(("de-chained", *de_form(case, True), case.rng))
    else:
        out.add(("pso", *pso_form(case), case.rng))
        if case.graph:
            out.add(("pso", *pso_form(case, True), case.rng))
    return out


# ---- the table -----------------------------------------------------------------------------------------------------------
# A trial of rand1bin / rand2bin with the default mutation 0.5 is a worse point than a random one: in a run of GENS
# generations from a random population of a few dozen rows no row ever wins.  With a short difference vector the trial's
# elements are as good as another row's, and about half the rows win; best2bin, with two difference vectors, likewise.
DE_MUTATION = {"rand1bin": 0.1, "rand2bin": 0.1, "best2bin": 0.3, "best1bin": 0.5}


# Likewise a particle of the default swarm overshoots the best position by up to a half, which x^4 punishes: on
# styblinski_tang with rows of 128 elements and more no particle improves in GENS generations.  A swarm that contracts does.
CONTRACTING = {"cognitivity": 1.0, "sociability": 0.7}


def _case(method, objective, n, pop, rng="philox", kind="run", graph=False, restart=False, seed=None, **options):
    if method == "de":
        options.setdefault("mutation", DE_MUTATION[options["strategy"]])
    elif objective == "styblinski_tang" and options.get("constraints") is None:
        options = dict(CONTRACTING, **options)
    what = [method, objective, "n%d" % n, str(pop), "host" if rng == "numpy-legacy" else "philox"]
    what += [str(options[k]) for k in ("strategy", "constraints") if options.get(k) is not None]
    what += [kind] if kind != "run" else []
    return Case("-".join(what), method, objective, n, pop, rng, options, kind, graph, restart, seed)


def _de_cases():
    out = []
    # A. the sweep: every objective at every row length of NS -- the general forms of both paths at 16 / 32 / 64 lanes (n = 3:
    #    fewer elements than lanes; 17, 100, 130, 200, 300: tail elements; 300: two batches) with ragged last workgroups, the
    #    strategies in rotation; with whole workgroups the FULL / NFIX forms at n = 64 / 128 / 256.  n = 17 / 100 / 200 on host
    #    draws (SX_RNG_HOST: two-kernel path only), so that every objective takes them in every lanes-per-row class.
    for oi, objective in enumerate(ALL):
        for ni, n in enumerate(NS):
            out.append(_case("de", objective, n, ("ragged", "whole")[(ni + oi // 2) % 2],
                             "numpy-legacy" if n in HOST_NS else "philox", strategy=STRATEGIES[(oi + ni) % 4]))
    # B. NFIX: the four hot objectives at the compile-time row lengths with whole workgroups, under each strategy -- best1bin /
    #    rand1bin: NFIX+STRAT; rand2bin / best2bin: NFIX with the run-time strategy.  (Two-kernel path: STRAT, ONEB at n = 256,
    #    general.)  One n per (objective, strategy) keeps the graph runs few: the chunked replays of every NFIX form.
    for oi, objective in enumerate(HOT):
        for n in (64, 128, 256):
            for si, strategy in enumerate(STRATEGIES):
                out.append(_case("de", objective, n, "whole", strategy=strategy,
                                 graph=(oi + si) % 4 == (64, 128, 256).index(n)))
    # C. the same shapes with the non-hot objectives: FULL with the run-time row length
    for oi, objective in enumerate(COLD):
        for ni, n in enumerate((64, 128, 256)):
            out.append(_case("de", objective, n, "whole", strategy=STRATEGIES[(oi + ni + 1) % 4], graph=oi == ni))
    # D. long rows.  n = 512 / 1024 with whole workgroups: FULL, compile-time summation plan, hot and non-hot; n = 700: the
    #    run-time plan (three batches, the last partial), a cosine objective and quartic
    for n in (512, 1024):
        for oi, objective in enumerate(("rosenbrock", "rastrigin", "griewank", "quartic")):
            out.append(_case("de", objective, n, "whole", strategy=STRATEGIES[(oi + n // 512) % 4],
                             graph=(n, objective) in ((512, "griewank"), (1024, "rastrigin"))))
    out.append(_case("de", "rastrigin", 700, "ragged", strategy="best1bin", graph=True))
    out.append(_case("de", "quartic", 700, "ragged", strategy="rand2bin"))
    # E. ONEB: whole-wave rows of run-time length with a hot objective, best1bin / rand1bin, constraints=None (both paths)
    for oi, objective in enumerate(HOT):
        for si, strategy in enumerate(SPECIAL_STRATEGIES):
            out.append(_case("de", objective, (130, 200)[(oi + si) % 2], "ragged", strategy=strategy, graph=oi == 2 * si))
    # F. STRAT: short rows of run-time length, the same conditions
    for oi, objective in enumerate(HOT):
        for si, strategy in enumerate(SPECIAL_STRATEGIES):
            out.append(_case("de", objective, (17, 100)[(oi + si) % 2], "ragged", strategy=strategy, graph=oi == 2 * si + 1))
    # G. Random with mutation = 1.5 (repairs happen): a hot and a non-hot objective in every lanes-per-row class (general form:
    #    the repair code and, with Philox, the resample draws), the NFIX shapes (NFIX without STRAT), and host draws (the
    #    resample block the host drew)
    for n, strategy in ((17, "best1bin"), (100, "rand1bin"), (200, "best2bin")):
        out.append(_case("de", "rastrigin", n, "ragged", strategy=strategy, graph=n == 100, **RANDOM))
        out.append(_case("de", "styblinski_tang", n, "ragged", strategy=strategy, graph=n == 200, **RANDOM))
    for objective, n, strategy in (("sphere", 64, "best1bin"), ("ackley", 128, "rand2bin"), ("rosenbrock", 256, "rand1bin")):
        out.append(_case("de", objective, n, "whole", strategy=strategy, graph=n == 128, **RANDOM))
    for objective, n, strategy in (("ackley", 64, "rand1bin"), ("griewank", 128, "best1bin"), ("quartic", 300, "rand2bin")):
        out.append(_case("de", objective, n, "ragged", "numpy-legacy", strategy=strategy, **RANDOM))
    # H. stops: an ftol the run meets at generation STOP_GEN (status 1; with a large xtol: 0), per lanes-per-row class
    #    (seeds: runs whose best value falls at generation STOP_GEN itself -- the host test asserts it)
    for objective, n, strategy, seed in (("griewank", 17, "rand1bin", 7), ("ackley", 100, "best1bin", 2),
                                         ("rastrigin", 200, "best1bin", 1)):
        for kind in ("stop1", "stop0"):
            out.append(_case("de", objective, n, "ragged", kind=kind, seed=seed, strategy=strategy))
    return out


def _pso_cases():
    out = []
    # A. the sweep, constraints=None: PLAIN for the hot objectives and the general form for the others at every row length;
    #    n = 64 / 128 / 256: FULL+PLAIN and FULL; n = 130 / 300 hot: ONEB+PLAIN / PLAIN with two batches; host draws at
    #    n = 17 / 100 / 200 (general form whatever the objective)
    replayed = {("ackley", 3), ("griewank", 130), ("quartic", 64), ("rastrigin", 128), ("rosenbrock", 300), ("sphere", 256),
                ("styblinski_tang", 128)}
    for oi, objective in enumerate(ALL):
        for ni, n in enumerate(NS):
            out.append(_case("pso", objective, n, ("ragged", "whole")[(ni + oi // 2) % 2],
                             "numpy-legacy" if n in HOST_NS else "philox", graph=(objective, n) in replayed))
    # B. Shrink with inertia 1, cognitivity = sociability = 3 (particles leave the box, beta < 1): hot and non-hot, every class,
    #    FULL at n = 64 / 128 / 256, ONEB at n = 200, and host draws
    for objective, ns in (("rosenbrock", (17, 128, 200)), ("ackley", (64, 100, 256)), ("griewank", (17, 128, 256)),
                          ("quartic", (64, 100, 200))):
        for n in ns:
            out.append(_case("pso", objective, n, "ragged" if n in (17, 100, 200) else "whole", graph=n in (128, 200),
                             **SHRINK))
    out.append(_case("pso", "rastrigin", 100, "ragged", "numpy-legacy", **SHRINK))
    out.append(_case("pso", "styblinski_tang", 130, "ragged", "numpy-legacy", **SHRINK))
    # C. cpso on whole-batch rows: FULL+PLAIN / FULL stepwise, and inside the replayed graph the radius by-product (FULL+RAD)
    for oi, objective in enumerate(("sphere", "rastrigin", "styblinski_tang")):
        for ni, n in enumerate((64, 128, 256)):
            out.append(_case("cpso", objective, n, "whole", graph=oi == ni))
    out.append(_case("cpso", "ackley", 128, "ragged", graph=True, **SHRINK))
    # D. ONEB: whole-wave rows of run-time length, hot objectives, Philox draws (the sweep runs n = 200 on host draws); and for
    #    the same reason n = 100 on Philox draws: PLAIN and the general form at 32 lanes per row
    for oi, objective in enumerate(HOT):
        out.append(_case("pso", objective, (200, 130)[oi % 2], "ragged", graph=oi == 0))
    out.append(_case("pso", "rosenbrock", 100, "ragged"))
    out.append(_case("pso", "ackley", 100, "whole", graph=True))
    out.append(_case("pso", "griewank", 100, "ragged", graph=True))
    out.append(_case("cpso", "sphere", 200, "ragged", graph=True))  # ... carrying the restart: ONEB without PLAIN
    # E. cpso with restarts that fire (256 particles: the swarm radius is below delta from the start), a hot and a non-hot
    #    objective, every lanes-per-row class, both draws
    out.append(_case("cpso", "ackley", 16, 256, restart=True, graph=True))
    out.append(_case("cpso", "quartic", 16, 256, restart=True, graph=True))
    out.append(_case("cpso", "griewank", 100, 256, restart=True))
    out.append(_case("cpso", "rastrigin", 200, 256, restart=True, graph=True))
    out.append(_case("cpso", "ackley", 16, 256, "numpy-legacy", restart=True))
    out.append(_case("cpso", "styblinski_tang", 64, 256, restart=True, graph=True, **SHRINK))
    # F. stops, per lanes-per-row class (a contracting swarm: the default one's best value does not fall at generation STOP_GEN)
    for objective, n, seed in (("rastrigin", 17, 9), ("griewank", 100, 1), ("ackley", 200, 2)):
        for kind in ("stop1", "stop0"):
            out.append(_case("pso", objective, n, "ragged", kind=kind, seed=seed, **CONTRACTING))
    return out


def _unique(cases):
    """A case two groups both name runs once (replayed as a graph if either asks for it)."""
    out = {}
    for c in cases:
        out[c.tag] = c._replace(graph=c.graph or out[c.tag].graph) if c.tag in out else c
    return list(out.values())


CASES = _unique(_de_cases() + _pso_cases())
BY_TAG = {c.tag: c for c in CASES}
PHILOX_CASES = [c for c in CASES if c.rng == "philox"]
GRAPH_CASES = [c for c in CASES if c.graph]
STOP_CASES = [c for c in CASES if c.kind != "run"]
assert all(c.rng == "philox" for c in GRAPH_CASES + STOP_CASES)


# ---- the reference -------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple(
    "Reference", "res pops pops_after best_x best_f cand_f fit fit_after restarts")


def oracle_run(case, objective, maxiter=GENS, ftol=-1.0, xtol=0.0):
    """The oracle's run of the case with `objective` (a callable on (P, n) arrays) and everything the comparisons read:
      pops[g - 1]        the population the callback sees after generation g (cpso: before that generation's restart);
      pops_after[g - 1]  the same after the restart (what the device holds when the next generation starts);
      best_x, best_f     the best row and value after generation g;
      cand_f[g - 1]      the candidates' values of generation g (generation 1: the initial population's);
      fit[g - 1]         the fitness vector after selection (DE: of the population; PSO: of the personal bests);
      fit_after[g - 1]   ... after the restart (restarted rows: 1e30)."""
    pops, live, best_x, best_f, cand_f = [], [], [], [], []

    def fun(X):
        f = np.asarray(objective(X), dtype=np.float64)
        cand_f.append(f.copy())
        return f

    def callback(X, r):
        pops.append(X.copy())
        live.append(X)  # (the PSO loop re-seeds restarted rows of this very array after the callback)
        best_x.append(np.array(r.x, copy=True))
        best_f.append(float(r.fun))

    res = oracle.minimize(fun, bounds(case), method=case.method, rng=case.rng, callback=callback,
                          options=dict(run_options(case, maxiter, ftol, xtol), return_all=True, verbosity=1.0))
    assert len(pops) == len(cand_f) == res.nit
    restarts = dict(zip((it for it, _ in res.get("_restarts", ())), res.get("_restart_rows", ())))
    fit, fit_after, cur = [], [], cand_f[0].copy()
    for g in range(1, res.nit + 1):
        if g > 1:
            cur = np.where(cand_f[g - 1] < cur, cand_f[g - 1], cur)  # _common.py:127, strict <
        fit.append(cur.copy())
        if g in restarts:
            cur = cur.copy()
            cur[restarts[g]] = 1.0e30
        fit_after.append(cur.copy())
    pops_after = [X.copy() if case.method != "de" else P for X, P in zip(live, pops)]
    for a in pops + pops_after + best_x + cand_f + fit + fit_after:
        a.setflags(write=False)
    return Reference(res, pops, pops_after, best_x, best_f, cand_f, fit, fit_after, restarts)


def stop_ftol(free):
    """The ftol of a stop case: the free run's best value at generation STOP_GEN."""
    return float(free.best_f[STOP_GEN - 1])


def stop_settings(case, free):
    """(ftol, xtol) of the stop case's second run: status 1 with xtol = 0, status 0 with an xtol no step exceeds."""
    return stop_ftol(free), (0.0 if case.kind == "stop1" else 1.0e3)


def case_run(case, objective, maxiter=GENS):
    """The run the case is about: the free run, or for a stop case the run under the ftol its free run gives."""
    free = oracle_run(case, objective, maxiter)
    if case.kind == "run":
        return free
    ftol, xtol = stop_settings(case, free)
    return oracle_run(case, objective, maxiter, ftol, xtol)


def case_settings(case, objective):
    """(ftol, xtol) the device is given for the case."""
    if case.kind == "run":
        return -1.0, 0.0
    return stop_settings(case, oracle_run(case, objective))


# ---- evidence, on the oracle alone -----------------------------------------------------------------------------------------
@contextlib.contextmanager
def _spied(name, wrap):
    """`oracle.engine.<name>` replaced by `wrap(original)` for the duration (the loops look the name up at every call)."""
    original = getattr(engine, name)
    setattr(engine, name, wrap(original))
    try:
        yield
    finally:
        setattr(engine, name, original)


def evidence(case):
    """What the case exercises, counted on the oracle's run with the numpy objective: per generation the number of winning
    rows, the elements Random repaired, the rows Shrink scaled (beta < 1); the restarts; the run itself."""
    repaired, scaled = [], []

    def count_repairs(original):
        def de_candidates(X, gbest, draws, F, CR, strategy, lower, upper, constraints):
            raw = original(X, gbest, draws, F, CR, strategy, lower, upper, None)
            repaired.append(int(((raw < lower) | (raw > upper)).sum()))
            return original(X, gbest, draws, F, CR, strategy, lower, upper, constraints)

        return de_candidates

    def count_scaled(original):
        def shrink_factor(X, V, lower, upper):
            beta = original(X, V, lower, upper)
            scaled.append(int((beta < 1.0).sum()))
            return beta

        return shrink_factor

    with _spied("de_candidates", count_repairs), _spied("shrink_factor", count_scaled):
        ref = case_run(case, OBJECTIVES[case.objective])
    wins = [int((ref.cand_f[g] < ref.fit_after[g - 1]).sum()) for g in range(1, ref.res.nit)]
    return dict(ref=ref, wins=wins, repaired=repaired, scaled=scaled, restarts=ref.restarts)


# ---- the device's launch forms ---------------------------------------------------------------------------------------------
def device_objective(sa, case):
    handle = getattr(sa.factory, case.objective)
    return lambda X: handle(X)


@functools.lru_cache(maxsize=None)
def _device_reference(tag, maxiter):
    import stochopy_amd as sa

    case = BY_TAG[tag]
    return case_run(case, device_objective(sa, case), maxiter)


def device_reference(case, maxiter=GENS):
    """The oracle's run on the device's own objective values, computed once per case and shared (read-only)."""
    return _device_reference(case.tag, maxiter)


@functools.lru_cache(maxsize=None)
def _device_settings(tag):
    import stochopy_amd as sa

    case = BY_TAG[tag]
    return case_settings(case, device_objective(sa, case))


def minimize_on_device(sa, case, maxiter=GENS, watch=True):
    """`stochopy_amd.optimize.minimize` of the case: (result, the populations its callback saw).  `watch`: with a callback
    and return_all (the two-kernel path, one generation per launch); without: the path that enqueues ahead."""
    ftol, xtol = _device_settings(case.tag)
    pops = []
    more = dict(return_all=True, verbosity=1.0) if watch else {}
    res = sa.optimize.minimize(getattr(sa.factory, case.objective), bounds(case), method=case.method,
                               options=dict(run_options(case, maxiter, ftol, xtol), backend="hip", rng=case.rng, **more),
                               callback=(lambda X, r: pops.append(np.array(X, copy=True))) if watch else None)
    return res, pops


def make_run(case, maxiter=GENS):
    """The case's `_DeRun` / `_PsoRun`, not yet set up (Philox draws, nothing watching: DE takes the chained kernel)."""
    from stochopy_amd import _lib
    from stochopy_amd.optimize import _cpso, _de

    ftol, xtol = _device_settings(case.tag)
    o, n = case.options, case.n
    lower, upper = np.full(n, -BOUND), np.full(n, BOUND)
    common = (xtol, ftol, False, 1.0, None, "philox", seed_of(case), 1)
    if case.method == "de":
        run = _de._DeRun(_lib.FUN_IDS[case.objective], lower, upper, None, maxiter, popsize(case), o.get("mutation", 0.5),
                         o.get("recombination", 0.9), o["strategy"], o.get("constraints"), *common, autorun=False)
        assert run.chain, "the case must take the chained kernel"
        return run
    gamma = o.get("competitivity", 1.0) if case.method == "cpso" else None
    return _cpso._PsoRun(_lib.FUN_IDS[case.objective], lower, upper, None, maxiter, popsize(case), o.get("inertia", 0.7298),
                         o.get("cognitivity", 1.49618), o.get("sociability", 1.49618), gamma, o.get("constraints"), *common,
                         autorun=False)


def _snapshot(run, st):
    """Everything a launch behind the stop could write to: both generations' rows, the fitness vector, the state."""
    rows = [b.cpu().numpy() for b in run.bufs] if hasattr(run, "bufs") else [t.cpu().numpy() for t in (run.X, run.V, run.pbest)]
    fit = (run.fit if hasattr(run, "bufs") else run.pbestfit).cpu().numpy()
    return rows, fit, (int(st.it), int(st.gbidx), float(st.gfit), int(st.status), int(st.done))


def stepwise(run, gens):
    """Generation 1 and the ones after it, one `enqueue(1)` each, until the run is done (at most `gens` generations), and one
    more launch behind the end: ([(state, population, fitness vector, best row)], the status the run settles on, snapshot
    before that launch, snapshot after)."""
    import torch

    def look():
        st = run.read_state()
        fit = run.fit if hasattr(run, "bufs") else run.pbestfit
        return st, run._population(st.it).cpu().numpy(), fit.cpu().numpy(), np.array(run._best_row(st), copy=True)

    out = []
    with torch.cuda.stream(run.ctx.stream):
        run._setup()
        out.append(look())
        while not out[-1][0].done and len(out) < gens:
            run.enqueue(1)
            out.append(look())
        status = run._settle_status(out[-1][0]) if out[-1][0].done else None
        before = _snapshot(run, out[-1][0])
        run.enqueue(1)
        after = _snapshot(run, run.read_state())
    return out, status, before, after


def same_snapshot(a, b):
    return (a[2] == b[2] and np.array_equal(a[1], b[1]) and len(a[0]) == len(b[0])
            and all(np.array_equal(u, v) for u, v in zip(a[0], b[0])))


def first_difference(got, want):
    """Where two populations (or vectors) differ first, for a failure message."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "shapes %s and %s" % (got.shape, want.shape)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    if bad.size == 0:
        return "equal"
    where = tuple(int(i) for i in bad[0])
    rows = np.unique(bad[:, 0]).size
    return "%d row(s) differ, first at %s: %r, expected %r" % (rows, where, got[where], want[where])
