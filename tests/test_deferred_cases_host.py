"""The table of tests/_deferred_cases.py exercises what it claims -- shown on the oracle alone, with the numpy objectives,
so that the GPU test's bit-for-bit comparisons (tests/test_gpu_deferred_forms.py) are known to pass through both branches of
every selection, through repairs, scaled rows, restarts and stops, and through every form of the two `pick_kernel`
dispatchers.  Runs on the CPU; the library is loaded only for sx_rows_per_workgroup."""
import collections
import functools

import numpy as np
import pytest

import _deferred_cases as dc
from oracle.objectives import OBJECTIVES

TAG = lambda c: c.tag  # noqa: E731
CLASSES = (16, 32, 64)


@functools.lru_cache(maxsize=None)
def evidence(tag):
    return dc.evidence(dc.BY_TAG[tag])


def constraints(case):
    return case.options.get("constraints")


@pytest.mark.parametrize("case", dc.CASES, ids=TAG)
def test_case_is_a_short_run_over_two_workgroups_or_more(case):
    P, rows = dc.popsize(case), dc.rows_per_workgroup(case.n)
    assert P > rows, "more than one workgroup"
    assert case.pop != "whole" or P == 2 * rows
    assert case.pop != "ragged" or (P == 2 * rows + 3 and P % rows != 0)
    assert case.method != "de" or P - 1 >= {"rand1bin": 3, "rand2bin": 5, "best1bin": 2, "best2bin": 4}[case.options["strategy"]]
    ref = evidence(case.tag)["ref"]
    assert ref.res.nit <= dc.GENS and len(ref.pops) == ref.res.nit
    if case.kind == "run":
        assert (ref.res.nit, ref.res.status) == (dc.GENS, -1)


@pytest.mark.parametrize("case", dc.CASES, ids=TAG)
def test_case_has_a_generation_with_winners_and_losers(case):
    """Both sides of `fc < fold` in one launch: some rows replaced, some kept."""
    wins, P = evidence(case.tag)["wins"], dc.popsize(case)
    assert any(0 < w < P for w in wins), wins


@pytest.mark.parametrize("case", [c for c in dc.CASES if constraints(c) == "Random"], ids=TAG)
def test_random_case_repairs_elements(case):
    repaired = evidence(case.tag)["repaired"]
    assert len(repaired) == dc.GENS - 1 and sum(repaired) >= 1, repaired
    assert sum(r > 0 for r in repaired) >= 2, repaired  # (not a single stray element)


@pytest.mark.parametrize("case", [c for c in dc.CASES if constraints(c) == "Shrink"], ids=TAG)
def test_shrink_case_scales_rows(case):
    """beta < 1 for some rows and -- in some generation -- not for all of them: both sides of Shrink's row-wide minimum."""
    scaled, P = evidence(case.tag)["scaled"], dc.popsize(case)
    assert sum(scaled) >= 1, scaled
    assert any(0 < s < P for s in scaled), scaled


@pytest.mark.parametrize("case", [c for c in dc.CASES if c.restart], ids=TAG)
def test_restart_case_restarts(case):
    restarts = evidence(case.tag)["restarts"]
    assert len(restarts) >= 1 and all(len(rows) >= 1 for rows in restarts.values())
    assert all(2 <= it < dc.GENS for it in restarts)
    if case.graph:  # ... and in the run of GRAPH_GENS generations as well (delta depends on maxiter)
        assert len(dc.case_run(case, OBJECTIVES[case.objective], dc.GRAPH_GENS).restarts) >= 1


@pytest.mark.parametrize("case", dc.STOP_CASES, ids=TAG)
def test_stop_case_ends_where_the_table_says(case):
    """The free run's best value falls at generation STOP_GEN, so under that ftol the run ends there and not before: with
    status 1 (the best row moved: xtol = 0), or 0 under an xtol no step exceeds."""
    free = dc.oracle_run(case, OBJECTIVES[case.objective])
    assert free.res.nit == dc.GENS and free.res.status == -1
    assert free.best_f[dc.STOP_GEN - 1] < free.best_f[dc.STOP_GEN - 2]
    assert free.best_f[-1] < free.best_f[dc.STOP_GEN - 1], "the free run goes on improving: the stop cuts something off"
    ref = evidence(case.tag)["ref"]
    assert (ref.res.nit, ref.res.status) == (dc.STOP_GEN, 1 if case.kind == "stop1" else 0)
    assert case.objective in dc.INEXACT and case.rng == "philox"
    for a, b in zip(ref.pops, free.pops):
        assert np.array_equal(a, b)


def test_stop_cases_cover_every_method_and_class():
    seen = {(("de" if c.method == "de" else "pso"), dc.lanes_per_row(c.n), c.kind) for c in dc.STOP_CASES}
    assert seen == {(m, k, s) for m in ("de", "pso") for k in CLASSES for s in ("stop1", "stop0")}


def test_every_objective_in_every_class_on_both_draws_ragged_and_whole():
    for family in ("de", "pso"):
        cases = [c for c in dc.CASES if (c.method == "de") == (family == "de")]
        seen = collections.Counter((c.objective, dc.lanes_per_row(c.n), c.rng) for c in cases)
        for objective in dc.ALL:
            for k in CLASSES:
                for rng in ("philox", "numpy-legacy"):
                    assert seen[objective, k, rng] >= 1, (family, objective, k, rng)
            pops = {c.pop for c in cases if c.objective == objective}
            assert {"ragged", "whole"} <= pops, (family, objective)


def test_every_objective_under_every_strategy():
    seen = collections.Counter((c.objective, c.options["strategy"]) for c in dc.CASES if c.method == "de")
    for objective in dc.ALL:
        for strategy in dc.STRATEGIES:
            assert seen[objective, strategy] >= 1, (objective, strategy)


def test_every_row_length_the_issue_names():
    de = {c.n for c in dc.CASES if c.method == "de"}
    assert set(dc.NS) | {512, 700, 1024} <= de
    for objective in dc.ALL:
        assert {c.n for c in dc.CASES if c.method == "de" and c.objective == objective} >= {3, 17, 64, 100, 128, 130, 200, 256, 300}
        assert {c.n for c in dc.CASES if c.method != "de" and c.objective == objective} >= {3, 17, 64, 100, 128, 130, 200, 256, 300}


def test_every_form_of_both_dispatchers():
    seen = set()
    for c in dc.CASES:
        seen |= dc.forms(c)
    want = set()
    for k in CLASSES:
        want |= {("de-chained", f, k, "philox") for f in ("general", "STRAT", "FULL", "NFIX", "NFIX+STRAT")}
        want |= {("de-two-kernel", f, k, "philox") for f in ("general", "STRAT")}
        want |= {("de-two-kernel", "general", k, "numpy-legacy"), ("pso", "general", k, "numpy-legacy")}
        want |= {("pso", f, k, "philox") for f in ("general", "PLAIN", "FULL", "FULL+PLAIN", "FULL+RAD")}
    want |= {("de-chained", "ONEB", 64, "philox"), ("de-two-kernel", "ONEB", 64, "philox"), ("pso", "ONEB", 64, "philox"),
             ("pso", "ONEB+PLAIN", 64, "philox")}
    assert want <= seen, sorted(want - seen)
    # one replayed-graph run per form
    graphs = set()
    for c in dc.GRAPH_CASES:
        graphs |= {(f[0], f[1]) for f in dc.forms(c) if f[0] != "de-two-kernel"}
    assert graphs >= {("de-chained", f) for f in ("general", "STRAT", "ONEB", "FULL", "NFIX", "NFIX+STRAT")}
    assert graphs >= {("pso", f) for f in ("general", "PLAIN", "FULL", "FULL+PLAIN", "FULL+RAD", "ONEB", "ONEB+PLAIN")}


def test_nfix_under_each_strategy_and_full_with_the_other_objectives():
    """The four hot objectives at n = 64 / 128 / 256 with whole workgroups under each of the four strategies; the same shapes
    with every non-hot objective; n = 512 and 1024 hot and non-hot; n = 700 for a cosine objective and quartic."""
    plain = [c for c in dc.CASES if c.method == "de" and c.rng == "philox" and c.pop == "whole" and constraints(c) is None]
    for n in (64, 128, 256):
        for objective in dc.HOT:
            for strategy in dc.STRATEGIES:
                hit = [c for c in plain if (c.objective, c.n, c.options["strategy"]) == (objective, n, strategy)]
                assert hit and dc.de_form(hit[0], True)[0] == ("NFIX+STRAT" if strategy in dc.SPECIAL_STRATEGIES else "NFIX")
        for objective in dc.COLD:
            hit = [c for c in plain if (c.objective, c.n) == (objective, n)]
            assert hit and dc.de_form(hit[0], True)[0] == "FULL", (objective, n)
    for n in (512, 1024):
        got = {c.objective for c in plain if c.n == n and dc.de_form(c, True)[0] == "FULL"}
        assert got & set(dc.HOT) and got & set(dc.COLD), (n, got)
    long = {c.objective for c in dc.CASES if c.method == "de" and c.n == 700}
    assert "quartic" in long and long & {"ackley", "rastrigin"}


def test_random_and_shrink_cover_hot_and_other_objectives():
    rnd = [c for c in dc.CASES if constraints(c) == "Random"]
    for k in CLASSES:
        assert any(c.objective in dc.HOT and dc.lanes_per_row(c.n) == k and c.rng == "philox" for c in rnd)
        assert any(c.objective in dc.COLD and dc.lanes_per_row(c.n) == k and c.rng == "philox" for c in rnd)
        assert any(dc.lanes_per_row(c.n) == k and c.rng == "numpy-legacy" for c in rnd)
        assert any(c.rng == "philox" and dc.de_form(c, True) == ("NFIX", k) for c in rnd)
    assert all(c.options["mutation"] == 1.5 for c in rnd)
    shr = [c for c in dc.CASES if constraints(c) == "Shrink"]
    assert all((c.options["inertia"], c.options["cognitivity"], c.options["sociability"]) == (1.0, 3.0, 3.0) for c in shr)
    for k in CLASSES:
        assert any(c.objective in dc.HOT and dc.lanes_per_row(c.n) == k for c in shr)
        assert any(c.objective in dc.COLD and dc.lanes_per_row(c.n) == k for c in shr)
    assert {c.rng for c in shr} == {"philox", "numpy-legacy"}


def test_cpso_cases():
    cpso = [c for c in dc.CASES if c.method == "cpso"]
    assert {c.n for c in cpso if c.graph and dc.pso_form(c, True)[0] == "FULL+RAD"} == {64, 128, 256}
    firing = [c for c in cpso if c.restart]
    assert any(c.objective == "ackley" for c in firing) and any(c.objective in dc.COLD for c in firing)
    assert {c.rng for c in firing} == {"philox", "numpy-legacy"}
    assert {dc.lanes_per_row(c.n) for c in firing} == set(CLASSES)


def test_dispatch_restatement_at_the_named_shapes():
    """`de_form` / `pso_form` on shapes whose kernel the sources name in their comments."""
    mk = dc._case
    assert dc.de_form(mk("de", "rosenbrock", 128, "whole", strategy="best1bin"), True) == ("NFIX+STRAT", 32)
    assert dc.de_form(mk("de", "rosenbrock", 128, "ragged", strategy="best1bin"), True) == ("STRAT", 32)
    assert dc.de_form(mk("de", "rosenbrock", 128, "whole", strategy="best1bin"), False) == ("STRAT", 32)
    assert dc.de_form(mk("de", "rosenbrock", 200, 24, strategy="best1bin"), True) == ("ONEB", 64)
    assert dc.de_form(mk("de", "rosenbrock", 100, 40, strategy="best1bin"), True) == ("STRAT", 32)
    assert dc.de_form(mk("de", "quartic", 128, "whole", strategy="best1bin"), True) == ("FULL", 32)
    assert dc.de_form(mk("de", "sphere", 512, "whole", strategy="rand2bin"), True) == ("FULL", 64)
    assert dc.de_form(mk("de", "sphere", 128, "whole", strategy="best1bin", **dc.RANDOM), True) == ("NFIX", 32)
    assert dc.de_form(mk("de", "sphere", 128, "whole", "numpy-legacy", strategy="best1bin"), False) == ("general", 32)
    assert dc.pso_form(mk("pso", "sphere", 250, "ragged")) == ("ONEB+PLAIN", 64)
    assert dc.pso_form(mk("pso", "sphere", 300, "ragged")) == ("PLAIN", 64)
    assert dc.pso_form(mk("pso", "griewank", 300, "ragged")) == ("general", 64)
    assert dc.pso_form(mk("cpso", "sphere", 256, "whole"), True) == ("FULL+RAD", 64)
    assert dc.pso_form(mk("pso", "sphere", 256, "whole", "numpy-legacy")) == ("general", 64)
