"""What tests/test_sample_smc_kernels_host.py and tests/test_gpu_sample_smc_kernels.py share: the inputs on which the kernels
of method="smc" (csrc/sx_sample_smc.hip) are driven ONE CALL AT A TIME through the C ABI, and how those inputs are admitted.

A whole run (tests/test_gpu_sample_smc.py) gives a kernel only what the sampler itself produces.  Here the host writes the
values, the records, the ancestors and the particles a call reads, and tests/_smc_oracle.py's stage_once / gather_once /
mutate_once say what one call makes of them.  Every call holds several populations with different inputs, the one the case is
about in the middle: nothing may pass between workgroups.

Admission (the method of _smc_cases.admitted): a tolerance only means something where the restatement's own rounding stays
well inside it.  A case that is not exact by construction is restated twice, the second time with every weight and every
running sum (part 1) or every objective value (part 3) moved at random by one unit in the last place; it is admitted when
that keeps every ancestor / acceptance count and moves beta and log Z by at most 1e-9.  Otherwise its seed moves on, at most
8 times.  The restatement alone decides; the host test asserts that every case listed here admits.
"""
import collections

import numpy as np

import _smc_oracle as oracle
from _smc_cases import moved_by_at_most
from oracle import objectives

C = 3            # populations per stage / gather call
MIDDLE = 1       # the population a case is about
SENTINEL = -7    # what anc holds before a stage call
M = 3            # Metropolis steps per stage
SEED = 20240611  # the Philox seed of every call (the cases' own seeds plant the values)
KEY = (SEED & 0xFFFFFFFF, SEED >> 32)
WIDE_FROM = 2048  # sx_wide_from(), asserted on the device
NAN_SENTINEL = np.array([0x7FF8DEADBEEF0001], dtype=np.uint64).view(np.float64)[0]
TRIES = 8


def make_nudge():
    rs = np.random.RandomState(0)

    def nudge(v):
        v = np.asarray(v, dtype=np.float64)
        return np.nextafter(v, v + rs.choice([-1.0, 1.0], size=v.shape))

    return nudge


def box(n):
    """Every axis has its own box, so an element read with another element's bounds shows."""
    e = np.arange(n, dtype=np.float64)
    return -1.0 - e / 7.0, 2.0 + e / 3.0


# ---- part 1: the stage kernel --------------------------------------------------------------------------------------------------
# P on both sides of K = ceil(P / 1024) = 1 | 2 | 3, of one wave of threads, with tail threads that own nothing, and the most.
STAGE_P = (4, 5, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, oracle.MAX_PARTICLES)
CROSS_P = (65, 1025, 2049)
# profile: a constant | b two values, 0 and 1e6, one particle in seven low | c uniform in [0, 30] | d = c with NaN and +inf on
# the edges of a thread, of a wave and of the population | e one finite value, at P - 1.
# start: fresh (s = 1 on started records) | mid (s = 4 on records of stage 3: step 6 runs on planted counts) | closing (s = 4 on
# populations that ended after stage 3: step 6 alone) | stale (s = 4 on populations that ended after stage 1: nothing)
# dead: None | "none" (no finite value) | "neginf" (a -inf at P - 1)
StageCase = collections.namedtuple("StageCase", "profile P ess target start maxiter dead")
StageCase.__new__.__defaults__ = (0.5, 0.234, "fresh", 100, None)

STAGE_CASES = [StageCase(profile, P) for profile in "abcde" for P in STAGE_P]
STAGE_CASES += [StageCase(profile, P, ess=ess) for profile in "bc" for P in CROSS_P for ess in (0.05, 0.95)]  # (0.5: above)
STAGE_CASES += [StageCase("c", P, target=target, start="mid") for P in CROSS_P for target in (0.1, 0.234, 0.6)]
STAGE_CASES += [StageCase("d", P, ess=0.95, start="mid") for P in CROSS_P]
STAGE_CASES += [StageCase("c", P, start="mid", maxiter=4) for P in CROSS_P]       # s == maxiter with beta < 1: status -1
STAGE_CASES += [StageCase("c", P, start=start) for P in CROSS_P for start in ("closing", "stale")]
STAGE_CASES += [StageCase("c", P, start=start, dead=dead) for P in (1025, 2049) for start in ("fresh", "mid")
                for dead in ("none", "neginf")]
EXACT_PROFILES = "ae"  # (b is not: at ess = 0.5 and 0.95 the halving ends where the high particles weigh about 0.3, not 0)

MID = {"beta": (0.11, 0.37, 0.62), "logz": (-0.5, -3.25, 4.75), "scale": (1.3, 0.8, 0.45), "s": 4}


def stage_id(case):
    parts = [case.profile, "P%d" % case.P]
    if case.ess != 0.5:
        parts.append("ess%g" % case.ess)
    if case.start != "fresh":
        parts.append(case.start)
    if case.start == "mid" and case.maxiter == 100 and case.profile == "c" and case.dead is None:
        parts.append("target%g" % case.target)
    if case.maxiter != 100:
        parts.append("maxiter%d" % case.maxiter)
    if case.dead:
        parts.append("dead-" + case.dead)
    return "-".join(parts)


def edge_indices(P):
    """Where profile d plants: a thread's first and last particle and its neighbour's first, a wave's edge, the final plateau.
    (At P = 4 these are all the particles: the neighbour's first gives way, a population needs one finite value.)"""
    K = -(-P // oracle.THREADS)
    idx = sorted({i for i in (0, K - 1, K, 63 * K, 64 * K, P - 2, P - 1) if 0 <= i < P})
    if len(idx) == P:
        idx.remove(K)
    return idx


def _one_finite(P, where, value):
    v = np.where(np.arange(P) % 2 == 0, np.nan, np.inf)
    v[where] = value
    return v


def _two_values(P, phase):
    return np.where(np.arange(P) % 7 == phase, 0.0, 1.0e6)


def stage_values(case, seed):
    """F (C, P): the case's profile in the middle, other values on both sides (exact ones beside an exact profile)."""
    P = case.P
    rs = np.random.RandomState(seed)
    uniform = rs.uniform(0.0, 30.0, size=(C, P))
    if case.profile == "a":
        F = np.stack([_one_finite(P, 0, 1.5), np.full(P, 2.5), np.full(P, 7.0)])
    elif case.profile == "b":
        F = np.stack([np.full(P, 1.5), _two_values(P, seed % 4), _two_values(P, (seed + 1) % 4)])
    elif case.profile == "e":
        F = np.stack([np.full(P, 1.5), _one_finite(P, P - 1, 3.0), _one_finite(P, P // 2, -4.0)])
    else:
        F = uniform
        if case.profile == "d":
            for k, i in enumerate(edge_indices(P)):
                F[MIDDLE, i] = np.nan if k % 2 == 0 else np.inf
            F[0, P - 1], F[2, 0] = np.inf, np.nan
    if case.dead == "none":
        F[MIDDLE] = np.where(np.arange(P) % 3 == 0, np.nan, np.inf)
    elif case.dead == "neginf":
        F[MIDDLE, P - 1] = -np.inf
    return F


def stage_inputs(case, seed):
    """What one sx_smc_stage call reads: F (C, P), the records (C, 8), nacc (C, P), s, and the args' scalars."""
    P = case.P
    F = stage_values(case, seed)
    rs = np.random.RandomState(seed + 1000)
    nacc = rs.randint(0, M + 1, size=(C, P)).astype(np.int64)
    record = oracle.start_records(C, 0.9)
    s = 1
    if case.start != "fresh":
        s = MID["s"]
        record[:, oracle.ST_BETA], record[:, oracle.ST_LOGZ], record[:, oracle.ST_SCALE] = MID["beta"], MID["logz"], MID["scale"]
        record[:, oracle.ST_ESS], record[:, oracle.ST_ACCEPT], record[:, oracle.ST_COUNT] = (0.61, 0.52, 0.93), 0.25, 17.0
        record[:, oracle.ST_STAGES] = s - 1
        if case.start == "closing":
            record[:, oracle.ST_STATUS], record[:, oracle.ST_BETA] = (0.0, 0.0, -1.0), (1.0, 1.0, 0.62)
        if case.start == "stale":
            record[:, oracle.ST_STATUS], record[:, oracle.ST_STAGES] = (0.0, -1.0, -2.0), 1.0
    return {"F": F, "record": record, "nacc": nacc, "s": s, "P": P, "ess": case.ess, "target": case.target, "M": M,
            "maxiter": case.maxiter}


def restated_stage(inp, nudge=None):
    return oracle.stage_once(inp["F"], inp["record"], inp["s"], inp["P"], inp["ess"], inp["target"], inp["M"], inp["maxiter"],
                             KEY, inp["nacc"], 0, nudge)


_stage = {}


def stage_admitted(case):
    """(seed, inputs, (records, ancestors) of the restatement).  Computed once per case and left unchanged."""
    if case in _stage:
        return _stage[case]
    first = 100 * STAGE_CASES.index(case)
    for seed in range(first, first + TRIES):
        inp = stage_inputs(case, seed)
        rec, anc = restated_stage(inp)
        ok = True
        if case.profile not in EXACT_PROFILES:
            rec2, anc2 = restated_stage(inp, make_nudge())
            with np.errstate(invalid="ignore"):  # (-inf beside -inf)
                ok = np.array_equal(anc, anc2) and np.array_equal(rec[:, [0, 5, 6, 7]], rec2[:, [0, 5, 6, 7]]) and \
                    moved_by_at_most(rec[:, oracle.ST_BETA], rec2[:, oracle.ST_BETA], 1e-9) and \
                    moved_by_at_most(rec[:, oracle.ST_LOGZ], rec2[:, oracle.ST_LOGZ], 1e-9)
        if ok:
            _stage[case] = (seed, inp, (rec, anc))
            return _stage[case]
    raise AssertionError("no admissible seed for " + stage_id(case))


def resampling_is_sound(F, beta0, beta, anc):
    """What systematic resampling promises of one population, whatever the restatement says: ancestors non-decreasing and
    inside [0, P), none of weight 0, and no particle's count of children 1 or more away from P w / sum w."""
    P = len(F)
    anc = np.asarray(anc)
    assert np.all(np.diff(anc) >= 0) and anc[0] >= 0 and anc[-1] < P
    usable = np.isfinite(F)
    fmin = F[usable].min()
    with np.errstate(all="ignore"):
        w = np.where(usable, np.exp(-((beta - beta0) * (F - fmin))), 0.0)
    assert np.all(w[anc] > 0.0)
    children = np.bincount(anc, minlength=P)
    assert np.all(np.abs(children - P * w / w.sum()) < 1.0), float(np.max(np.abs(children - P * w / w.sum())))
    return True


# ---- part 2: the gather kernel -------------------------------------------------------------------------------------------------
GATHER_N = (1, 15, 16, 17, 32, 33, 130, WIDE_FROM)  # on both sides of one and two tiles of 16 axes, many tiles, the longest row
GATHER_P = (4, 15, 16, 17, 100)                     # below, at and off the 16 particles the threads of an axis take at a time
GATHER_SCALE = (1.3, 0.8, 0.45)
# the ancestors, and the population that takes no part in the call (its record names another stage)
GATHER_ANCS = (("identity", None), ("reversed", 2), ("random", 0), ("one", None), ("outside", 2))
GUARD_ROWS = 8  # rows kept before and after every array: an ancestor of -7 or P + 3 read unclamped stays in the allocation


def gather_inputs(n, P, s, kind, seed=0):
    """x (C, P, n), f (C, P), anc (C, P), records (C, 8) of one sx_smc_resample call."""
    rs = np.random.RandomState(1000 * n + 10 * P + seed)
    x = rs.uniform(-1.0, 2.0, size=(C, P, n)) * (1.0 + np.arange(n))
    f = rs.uniform(0.0, 30.0, size=(C, P))
    f[0, 0], f[1, P - 1], f[2, 1] = np.nan, np.inf, -0.0
    ident = np.tile(np.arange(P), (C, 1))
    if kind == "identity":
        anc = ident
    elif kind == "reversed":
        anc = ident[:, ::-1].copy()
    elif kind == "one":
        anc = np.tile(np.array([[P - 1], [0], [P // 2]]), (1, P))
    else:
        anc = np.sort(rs.randint(0, P, size=(C, P)), axis=1)
        if kind == "outside":
            anc[MIDDLE, [0, 1, P - 2, P - 1]] = [-1, SENTINEL, P, P + 3]
    record = oracle.start_records(C, 1.0)
    record[:, oracle.ST_SCALE], record[:, oracle.ST_BETA], record[:, oracle.ST_STAGES] = GATHER_SCALE, 0.37, s
    skip = dict(GATHER_ANCS)[kind]
    if skip is not None:
        record[skip, oracle.ST_STAGES] = s - 1
    return x, f, anc.astype(np.int32), record


# ---- part 3: the mutation kernel -----------------------------------------------------------------------------------------------
MUTATE_S, MUTATE_C, MUTATE_P, MUTATE_BETA = 3, 5, 5, 0.37
MUTATE_FROZEN = (1, 3)
MUTATE_N = (1, 3, 64, 65, 128, 129, 300)  # 16 lanes per row to n = 64, 32 to 128, 64 beyond
MUTATE_FUNS = ("ackley", "griewank", "quartic", "rastrigin", "rosenbrock", "sphere", "styblinski_tang")
# (objective, n): every objective at two widths, every width, every row form under at least three objectives.  (ackley and
# griewank are nearly flat on the middle widths of this box: every proposal inside it would be accepted.)
MUTATE_CASES = [("ackley", 1), ("ackley", 3), ("griewank", 3), ("griewank", 300), ("quartic", 64), ("quartic", 65),
                ("rastrigin", 65), ("rastrigin", 128), ("rosenbrock", 128), ("rosenbrock", 129), ("sphere", 129), ("sphere", 64),
                ("styblinski_tang", 300), ("styblinski_tang", 1)]
# step_e = MUTATE_STEP[n] * h_e: the share of the half-width at which 20 % to 80 % of the proposals leave the box on some axis
MUTATE_STEP = {1: 1.2, 3: 0.5, 64: 0.03, 65: 0.03, 128: 0.015, 129: 0.015, 300: 0.006}


def mutate_id(case):
    return "%s-n%d" % case


def mutate_inputs(case, seed):
    fun, n = case
    lower, upper = box(n)
    rs = np.random.RandomState(seed)
    x = lower + (upper - lower) * rs.uniform(0.0, 1.0, size=(MUTATE_C, MUTATE_P, n))
    with np.errstate(all="ignore"):
        f = np.asarray(objectives.OBJECTIVES[fun](x.reshape(-1, n)), dtype=np.float64).reshape(MUTATE_C, MUTATE_P)
    f[0, 1], f[0, 3], f[2, 0], f[2, 4] = np.nan, np.inf, np.inf, np.nan  # a NaN d accepts; so does d = +inf
    step = np.tile(MUTATE_STEP[n] * (0.5 * (upper - lower)), (MUTATE_C, 1)) * np.array([1.0, 0.5, 1.1, 2.0, 0.9])[:, None]
    live = np.array([c not in MUTATE_FROZEN for c in range(MUTATE_C)])
    record = oracle.start_records(MUTATE_C, 0.8)
    record[:, oracle.ST_BETA], record[:, oracle.ST_STAGES] = MUTATE_BETA, MUTATE_S
    for c in MUTATE_FROZEN:
        record[c] = [0.0, 1.0, -2.0, 0.7, 0.8, 0.3, MUTATE_S - 1, 4.0]
    return {"x": x, "f": f, "step": step, "live": live, "record": record, "lower": lower, "upper": upper, "n": n, "fun": fun}


def restated_mutation(inp, nudge=None, trace=None):
    f_ = objectives.OBJECTIVES[inp["fun"]]
    fun = f_ if nudge is None else (lambda X: nudge(f_(X)))
    return oracle.mutate_once(inp["x"], inp["f"], inp["step"], inp["record"][:, oracle.ST_BETA], inp["live"], MUTATE_S, M, KEY,
                              inp["lower"], inp["upper"], fun, 0, trace)


def mutation_shares(inp, trace):
    """(the share of the live particles' proposals outside the box, accepted steps, rejected steps inside the box)."""
    live = np.repeat(inp["live"], MUTATE_P)
    outside = np.concatenate([o[live] for o, _ in trace])
    accept = np.concatenate([a[live] for _, a in trace])
    return float(outside.mean()), int(accept.sum()), int((~outside & ~accept).sum())


def mutation_is_telling(shares):
    """The condition of the case table: 20 % to 80 % of the proposals leave the box, the rest are accepted AND rejected."""
    outside, accepted, rejected = shares
    return 0.2 <= outside <= 0.8 and accepted >= 1 and rejected >= 1


_mutate = {}


def mutate_admitted(case):
    """(seed, inputs, (x, f, nacc) of the restatement, shares): the first seed whose restated mutation keeps every acceptance
    and every particle under the nudge of the objective's values and is telling."""
    if case in _mutate:
        return _mutate[case]
    first = 100 * MUTATE_CASES.index(case)
    for seed in range(first, first + TRIES):
        inp = mutate_inputs(case, seed)
        trace = []
        x, f, nacc = restated_mutation(inp, trace=trace)
        x2, f2, nacc2 = restated_mutation(inp, make_nudge())
        shares = mutation_shares(inp, trace)
        if np.array_equal(nacc, nacc2) and np.array_equal(x, x2) and mutation_is_telling(shares):
            _mutate[case] = (seed, inp, (x, f, nacc), shares)
            return _mutate[case]
    raise AssertionError("no admissible seed for " + mutate_id(case))


# ---- part 4: the propose / decide pair -----------------------------------------------------------------------------------------
PAIR_N = (3, 64, 65, 128, 129, 300, WIDE_FROM)
PAIR_FUNS = ("sphere", "rastrigin", "styblinski_tang", "rosenbrock")
PAIR_OPTIONS = {"chains": 3, "particles": 21, "steps": 3, "maxiter": 3}  # 63 rows: a ragged last workgroup in every row form
PAIR_LONGEST = {"chains": 3, "particles": 8, "steps": 3, "maxiter": 2}
PAIR_BOUND = 5.12

# The frozen contract: four populations that end after stages 1, 8, 0 and 2, so that frozen populations meet later stages of
# both parities -- in a box that excludes the origin, which is what a buffer nobody wrote holds.
FROZEN_P, FROZEN_NDIM = 64, 3
FROZEN_BOUNDS = [[1.0 + 0.1 * e, 2.0 + 0.3 * e] for e in range(FROZEN_NDIM)]
FROZEN_CENTRE = (1.3, 1.5, 2.0)
FROZEN_OPTIONS = {"chains": 4, "particles": FROZEN_P, "steps": 3, "maxiter": 12}
FROZEN_SEEDS = (3, 4, 5)
FROZEN_STAGES, FROZEN_STATUSES = (1, 8, 0, 2), (0, 0, -2, 0)
FROZEN_GPU_SEED = 3


def frozen_values(X):
    """One rule for the restatement (a numpy array) and the device (a tensor): (4 P, 3) -> (4 P,), the same operations in the
    same order."""
    d0, d1, d2 = (X[:, e] - FROZEN_CENTRE[e] for e in range(FROZEN_NDIM))
    r2 = d0 * d0 + d1 * d1 + d2 * d2
    out = r2 * 6.0
    out[:FROZEN_P] = 2.5
    out[FROZEN_P:2 * FROZEN_P] = r2[FROZEN_P:2 * FROZEN_P] * 2000.0
    out[2 * FROZEN_P:3 * FROZEN_P] = float("nan")
    return out
