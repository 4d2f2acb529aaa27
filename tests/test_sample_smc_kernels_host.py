"""CPU: what tests/test_gpu_sample_smc_kernels.py stands on.  The restatement taken one step at a time (tests/_smc_oracle.py's
stage_once, gather_once, mutate_once) is the restated run tests/test_gpu_sample_smc.py trusts; every case of
tests/_smc_kernel_cases.py admits (the restatement's own rounding stays inside the tolerances the device is held to) and is the
case its name says: the exact profiles have their closed forms, the planted mutations leave the box and are accepted and
rejected in the shares the table promises, the mixed objective of the frozen contract ends its populations after stages of both
parities.  No device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _smc_cases as cases  # noqa: E402
import _smc_kernel_cases as kc  # noqa: E402
import _smc_oracle as oracle  # noqa: E402
from oracle import objectives  # noqa: E402

ST = oracle


# ---- 0. the restatement, one step at a time ------------------------------------------------------------------------------------
CHAINED = [case for case in cases.PARITY if case[:4] in (("sphere", 1, 4, 1), ("sphere", 2, 63, 3), ("griewank", 2, 100, 3),
                                                         ("sphere", 3, 1025, 3))]


@pytest.mark.parametrize("case", CHAINED, ids=cases.parity_id)
def test_the_three_steps_chained_are_the_restated_run(case):
    """From the particles of stage 0, stage_once -> gather_once -> mutate_once over explicit state give every stage of
    sample(record=True) bit for bit."""
    fun, bounds, opts = cases.parity_setup(case)
    want = oracle.sample(fun, bounds, dict(opts), record=True)
    Cn, P, M, maxiter = opts["chains"], opts["particles"], opts["steps"], opts["maxiter"]
    lower, upper = (np.array(v, dtype=np.float64) for v in np.transpose(bounds))
    n = len(lower)
    key = (opts["seed"] & 0xFFFFFFFF, opts["seed"] >> 32)
    x, f = want.x0.copy(), want.f0.copy()
    record = oracle.start_records(Cn, 2.38 / np.sqrt(n))
    nacc = np.zeros((Cn, P), dtype=np.int64)
    assert want.nit >= 1 and {c[2] for c in CHAINED} == {4, 63, 100, 1025}
    for s in range(1, want.nit + 1):
        record, anc = oracle.stage_once(f, record, s, P, 0.5, 0.234, M, maxiter, key, nacc)
        took = record[:, ST.ST_STAGES] == s
        assert np.array_equal(took, want.took[s - 1]) and np.array_equal(anc, want.ancs[s - 1])
        x, f, step = oracle.gather_once(x, f, anc, record[:, ST.ST_SCALE], lower, upper)
        assert np.array_equal(step[took], want.steps_[s - 1][took])
        x, f, nacc = oracle.mutate_once(x, f, step, record[:, ST.ST_BETA], took, s, M, key, lower, upper, objectives.OBJECTIVES[fun])
        assert np.array_equal(nacc, want.naccs[s - 1])
        assert np.array_equal(record[:, ST.ST_BETA], np.atleast_2d(want.betas)[:, s])
    record, _ = oracle.stage_once(f, record, want.nit + 1, P, 0.5, 0.234, M, maxiter, key, nacc)
    assert np.array_equal(record[:, ST.ST_LOGZ], np.atleast_1d(want.log_evidence))
    assert np.array_equal(record[:, ST.ST_STATUS], np.atleast_1d(want.statuses).astype(np.float64))
    assert np.array_equal(record[:, ST.ST_STAGES], np.atleast_1d(want.stages).astype(np.float64))
    last = np.atleast_1d(want.stages) == want.nit
    assert np.array_equal(record[last, ST.ST_COUNT], np.atleast_2d(want.counts)[last, -1].astype(np.float64))
    assert np.array_equal(record[last, ST.ST_ACCEPT], np.atleast_2d(want.accept_ratios)[last, -1])
    assert np.array_equal(x, np.reshape(want.xall, (Cn, P, n))) and np.array_equal(f, np.reshape(want.funall, (Cn, P)))


def test_a_population_that_ends_keeps_its_scale_and_a_population_is_alone_in_its_call():
    """stage_once follows the header for populations that have ended, and a population's step does not depend on the others."""
    case = kc.StageCase("c", 65, start="mid")
    inp = kc.stage_inputs(case, 5)
    rec, anc = kc.restated_stage(inp)
    alone = dict(inp, F=inp["F"][:1], record=inp["record"][:1], nacc=inp["nacc"][:1])
    rec0, anc0 = kc.restated_stage(alone)
    assert np.array_equal(rec0[0], rec[0]) and np.array_equal(anc0[0], anc[0])  # (population 0: the row that keys u is 0 in both)
    x, f, a, record = kc.gather_inputs(17, 15, 1, "random")
    lower, upper = kc.box(17)
    x1, f1, step = oracle.gather_once(x, f, a, record[:, ST.ST_SCALE], lower, upper)
    x2, f2, step2 = oracle.gather_once(x[1:2], f[1:2], a[1:2], record[1:2, ST.ST_SCALE], lower, upper)
    assert np.array_equal(x1[1], x2[0]) and np.array_equal(f1[1], f2[0], equal_nan=True) and np.array_equal(step[1], step2[0])


# ---- 1. the stage kernel's cases -----------------------------------------------------------------------------------------------
def test_the_case_tables_hold_what_they_promise():
    assert len({kc.stage_id(c) for c in kc.STAGE_CASES}) == len(kc.STAGE_CASES)
    for profile in "abcde":
        assert {c.P for c in kc.STAGE_CASES if c.profile == profile and c == kc.StageCase(profile, c.P)} == set(kc.STAGE_P)
    K = [-(-P // oracle.THREADS) for P in kc.STAGE_P]
    assert sorted(set(K)) == [1, 2, 3, 5, 16] and kc.STAGE_P[-1] == oracle.MAX_PARTICLES
    assert kc.edge_indices(2049) == [0, 2, 3, 189, 192, 2047, 2048] and kc.edge_indices(4) == [0, 2, 3]
    assert {n for _, n in kc.MUTATE_CASES} == set(kc.MUTATE_N) and {f for f, _ in kc.MUTATE_CASES} == set(kc.MUTATE_FUNS)
    for form in ((1, 3, 64), (65, 128), (129, 300)):
        assert len({f for f, n in kc.MUTATE_CASES if n in form}) >= 3


@pytest.mark.parametrize("case", kc.STAGE_CASES, ids=kc.stage_id)
def test_a_stage_case_admits_and_is_what_its_name_says(case):
    seed, inp, (rec, anc) = kc.stage_admitted(case)  # (raises where no seed admits)
    P, before, m = case.P, inp["record"], kc.MIDDLE
    first = 100 * kc.STAGE_CASES.index(case)
    assert first <= seed < first + kc.TRIES
    took = rec[:, ST.ST_STAGES] == inp["s"]
    F, beta0, logz0 = inp["F"][m], before[m, ST.ST_BETA], before[m, ST.ST_LOGZ]
    if case.start == "stale":
        assert np.array_equal(rec, before) and not took.any()
        return
    if case.start == "closing":
        changed = rec != before
        assert not took.any() and not changed[:, [0, 1, 2, 3, 4, 6]].any() and changed[:, [5, 7]].all()
        count = inp["nacc"].sum(axis=1)
        assert np.array_equal(rec[:, ST.ST_COUNT], count.astype(np.float64))
        assert np.array_equal(rec[:, ST.ST_ACCEPT], count / (float(P) * float(kc.M)))
        return
    if case.start == "mid":  # step 6 on the planted counts
        count = inp["nacc"].sum(axis=1)
        assert np.array_equal(rec[:, ST.ST_COUNT], count.astype(np.float64))
        r = count / (float(P) * float(kc.M))
        assert np.array_equal(rec[:, ST.ST_ACCEPT], r)
        scale = before[:, ST.ST_SCALE] * np.exp(r - case.target)
        assert np.array_equal(rec[took, ST.ST_SCALE], scale[took]) and np.all(scale != before[:, ST.ST_SCALE])
    if case.dead:
        assert list(rec[:, ST.ST_STATUS]) == [1.0, -2.0, 1.0] and rec[m, ST.ST_LOGZ] == -np.inf and list(took) == [True, False, True]
        assert np.array_equal(rec[m, [1, 3, 4, 6]], before[m, [1, 3, 4, 6]]) and np.array_equal(anc[m], np.arange(P))
        return
    assert took.all()
    for c in range(kc.C):
        assert kc.resampling_is_sound(inp["F"][c], before[c, ST.ST_BETA], rec[c, ST.ST_BETA], anc[c])
    if case.maxiter == inp["s"]:
        assert np.all(rec[:, ST.ST_BETA] < 1.0) and np.all(rec[:, ST.ST_STATUS] == -1.0)
    if case.profile == "a":
        assert rec[m, ST.ST_BETA] == 1.0 and rec[m, ST.ST_ESS] == 1.0 and rec[m, ST.ST_STATUS] == 0.0
        assert rec[m, ST.ST_LOGZ] == logz0 - (1.0 - beta0) * F[0] and np.array_equal(anc[m], np.arange(P))
    if case.profile == "b":
        assert set(np.unique(F)) == {0.0, 1.0e6} and abs((F == 0.0).mean() - 1.0 / 7.0) <= 1.0 / P
        if case.ess == 0.05:  # the low particles alone are enough: beta = 1, the weights exactly 1 and 0
            assert rec[m, ST.ST_BETA] == 1.0 and rec[m, ST.ST_LOGZ] == np.log(float((F == 0.0).sum()) / float(P))
            assert np.all(F[anc[m]] == 0.0)
        else:  # the halving ends where the high particles still weigh: beta of the order of 1e-6
            assert 1e-7 < rec[m, ST.ST_BETA] < 1e-5 and abs(rec[m, ST.ST_ESS] - case.ess) < 0.5 / P + 1e-9
    if case.profile == "d":
        planted = kc.edge_indices(P)
        assert not np.isfinite(F[planted]).any() and np.isfinite(np.delete(F, planted)).all() and np.isfinite(F).any()
        assert not np.isin(anc[m], planted).any()
    if case.profile == "e":
        assert np.all(anc[m] == P - 1) and np.isfinite(F).sum() == 1 and rec[m, ST.ST_STATUS] == 1.0
        assert rec[m, ST.ST_BETA] == beta0 + 2.0 ** -52 * (1.0 - beta0) and rec[m, ST.ST_ESS] == 1.0 / P
        assert rec[m, ST.ST_LOGZ] == logz0 + (np.log(1.0 / float(P)) - (rec[m, ST.ST_BETA] - beta0) * 3.0)


def test_the_soundness_check_tells():
    """resampling_is_sound refuses ancestors one particle off and an ancestor without weight."""
    _, inp, (rec, anc) = kc.stage_admitted(kc.StageCase("d", 1025))
    F, m = inp["F"][kc.MIDDLE], kc.MIDDLE
    args = (F, inp["record"][m, ST.ST_BETA], rec[m, ST.ST_BETA])
    assert kc.resampling_is_sound(*args, anc[m])
    heavy = int(np.argmax(np.bincount(anc[m])))
    twice = np.sort(np.concatenate([anc[m][anc[m] != heavy], np.full((anc[m] == heavy).sum(), anc[m].min())]))
    for bad in (np.minimum(anc[m] + 1, 1024)[::-1], twice, np.where(np.arange(1025) == 0, 0, anc[m])):
        with pytest.raises(AssertionError):
            kc.resampling_is_sound(*args, bad)


# ---- 2. the gather kernel's cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k, _ in kc.GATHER_ANCS])
def test_the_gather_cases(kind):
    n, P = 17, 15
    lower, upper = kc.box(n)
    x, f, anc, record = kc.gather_inputs(n, P, 2, kind)
    x1, f1, step = oracle.gather_once(x, f, anc, record[:, ST.ST_SCALE], lower, upper)
    rows = np.arange(kc.C)[:, None]
    assert np.array_equal(x1, x[rows, np.clip(anc, 0, P - 1)])
    assert np.isnan(f).sum() == 1 and np.isinf(f).sum() == 1
    skip = dict(kc.GATHER_ANCS)[kind]
    assert [c for c in range(kc.C) if record[c, ST.ST_STAGES] != 2] == ([] if skip is None else [skip])
    if kind == "one":  # a collapsed axis: the floor, in closed form
        assert np.allclose(step, np.array(kc.GATHER_SCALE)[:, None] * 1.0e-8 * (0.5 * (upper - lower)), rtol=1e-12, atol=0)
    if kind == "outside":
        assert list(anc[kc.MIDDLE, [0, 1, P - 2, P - 1]]) == [-1, -7, P, P + 3] and anc[[0, 2]].min() >= 0 and anc[[0, 2]].max() < P
        assert np.array_equal(x1[kc.MIDDLE, [0, 1]], x[kc.MIDDLE, [0, 0]]) and np.array_equal(x1[kc.MIDDLE, [P - 2, P - 1]], x[kc.MIDDLE, [P - 1, P - 1]])
        assert -kc.GUARD_ROWS <= kc.SENTINEL and 3 <= kc.GUARD_ROWS
    else:
        assert anc.min() >= 0 and anc.max() < P
    assert np.all(np.std(x[:, :, -1], axis=1) > 4.0 * np.std(x[:, :, 0], axis=1))  # (the axes differ: a mixed-up axis shows)


# ---- 3. the mutation kernel's cases --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", kc.MUTATE_CASES, ids=kc.mutate_id)
def test_a_mutation_case_admits_and_leaves_the_box_in_its_share(case):
    seed, inp, (x, f, nacc), shares = kc.mutate_admitted(case)
    outside, accepted, rejected = shares
    print("    %-22s seed %4d  outside %.2f  accepted %2d  rejected inside %2d" % (kc.mutate_id(case), seed, outside, accepted, rejected))
    assert 0.2 <= outside <= 0.8 and accepted >= 1 and rejected >= 1
    frozen = list(kc.MUTATE_FROZEN)
    assert np.array_equal(x[frozen], inp["x"][frozen]) and np.array_equal(f[frozen], inp["f"][frozen]) and not nacc[frozen].any()
    live = inp["live"]
    assert np.isnan(inp["f"][live]).sum() == 2 and np.isinf(inp["f"][live]).sum() == 2
    assert np.all((inp["x"] >= inp["lower"]) & (inp["x"] <= inp["upper"])) and np.all((x >= inp["lower"]) & (x <= inp["upper"]))
    assert (kc.MUTATE_S - 1) * kc.M + 1 != 1  # (the step's number is not its number inside the stage)


# ---- 4. the frozen contract's objective ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", kc.FROZEN_SEEDS)
def test_the_mixed_objective_ends_its_populations_after_stages_of_both_parities(seed):
    res = oracle.sample(kc.frozen_values, kc.FROZEN_BOUNDS, dict(kc.FROZEN_OPTIONS, seed=seed))
    assert tuple(res.stages) == kc.FROZEN_STAGES and tuple(res.statuses) == kc.FROZEN_STATUSES and res.nit == max(kc.FROZEN_STAGES)
    lower, upper = np.transpose(kc.FROZEN_BOUNDS)
    assert np.all(lower > 0.0)  # (the origin, what an unwritten buffer holds, is outside)
    for c, s0 in enumerate(kc.FROZEN_STAGES):  # every ended population meets a later stage of each parity
        later = set((s - s0) % 2 for s in range(s0 + 1, res.nit + 1))
        assert later == ({0, 1} if s0 < res.nit else set())
    assert np.all((res.xall >= lower) & (res.xall <= upper))
