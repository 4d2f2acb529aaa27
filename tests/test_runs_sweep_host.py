"""options["runs"] = R with per-run hyperparameters (a sweep), host side (no GPU): a sequence of R values for `mutation`,
`recombination`, `strategy` (de), `inertia`, `cognitivity`, `sociability` (pso, cpso), `competitivity` (cpso) or `sigma`
(cmaes, vdcma) is validated -- one helper, optimize/_runs.py per_run -- before a device is needed; a scalar behaves as it
always did; the method's _minimize_runs receives an array for a sequence and a float for everything else; and the four
sx_*_runs_sweep_launch entry points are declared, exported and bound."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, P = 3, 8

# method -> (ndim, the options that may be per run -> (a valid sweep of R values, lowest admitted, highest admitted))
NUMERIC = {
    "de": (5, {"mutation": ([0.3, 0.5, 0.9], 0.0, 2.0), "recombination": ([0.1, 0.5, 1.0], 0.0, 1.0)}),
    "pso": (5, {"inertia": ([0.4, 0.7, 1.0], 0.0, 1.0), "cognitivity": ([0.0, 1.5, 4.0], 0.0, 4.0),
                "sociability": ([1.0, 1.5, 2.0], 0.0, 4.0)}),
    "cpso": (5, {"inertia": ([0.4, 0.7, 1.0], 0.0, 1.0), "cognitivity": ([0.0, 1.5, 4.0], 0.0, 4.0),
                 "sociability": ([1.0, 1.5, 2.0], 0.0, 4.0), "competitivity": ([0.0, 1.0, 2.0], 0.0, 2.0)}),
    "cmaes": (6, {"sigma": ([0.1, 0.3, 1.5], None, None)}),
    "vdcma": (6, {"sigma": ([0.1, 0.3, 1.5], None, None)}),
}
CASES = [(method, name) for method, (_, table) in NUMERIC.items() for name in table]
MODULE = {"de": "_de", "pso": "_cpso", "cpso": "_cpso", "cmaes": "_cmaes", "vdcma": "_vdcma"}


@pytest.fixture(scope="module")
def lib():
    from stochopy_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def sa(lib):
    import stochopy_amd

    return stochopy_amd


def _call(sa, method, **changes):
    n = NUMERIC[method][0]
    opts = dict({"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox"}, **changes)
    if method in ("de", "pso", "cpso"):
        opts.setdefault("updating", "deferred")
    return sa.optimize.minimize(sa.factory.sphere, [[-3.0, 3.0]] * n, method=method, options=opts)


class Reached(Exception):
    """Raised in place of the method's _minimize_runs: every check of minimize() has passed, no device was touched."""

    def __init__(self, args):
        super().__init__("reached _minimize_runs")
        self.received = args


@pytest.fixture
def intercepted(sa, monkeypatch):
    """minimize() of every method stops where _minimize_runs would start, with what it was about to pass."""
    import importlib

    def stop(*args):
        raise Reached(args)

    for module in set(MODULE.values()):
        monkeypatch.setattr(importlib.import_module("stochopy_amd.optimize." + module), "_minimize_runs", stop)
    return sa


def _bad_element(lo, hi):
    """(what, an element the option does not admit) for a numeric option of range [lo, hi], or > 0 (lo is None)."""
    out = [("a bool", True), ("a string", "0.5"), ("None", None), ("nan", float("nan")), ("inf", float("inf")),
           ("-inf", -float("inf"))]
    if lo is None:
        return out + [("zero", 0.0), ("negative", -0.1)]
    return out + [("below the range", np.nextafter(lo, -1.0)), ("above the range", np.nextafter(hi, 10.0))]


# ---- sequences that are refused


@pytest.mark.parametrize("method,name", CASES)
def test_a_sequence_needs_runs(sa, method, name):
    good = NUMERIC[method][1][name][0]
    for runs in (None, 1):
        with pytest.raises(ValueError, match=f"(?s){name}.*runs|runs.*{name}"):
            _call(sa, method, runs=runs, seed=0, **{name: good})
    with pytest.raises(ValueError, match=f"(?s){name}.*runs|runs.*{name}"):  # (the option left out altogether)
        n = NUMERIC[method][0]
        sa.optimize.minimize(sa.factory.sphere, [[-3.0, 3.0]] * n, method=method,
                             options={"popsize": P, "maxiter": 4, "seed": 0, "rng": "philox", name: good})


@pytest.mark.parametrize("method,name", CASES)
def test_a_sequence_of_the_wrong_shape_is_refused(sa, method, name):
    good = NUMERIC[method][1][name][0]
    for bad in (good[:2], good + good[:1], [], np.array(good)[:2], [good, good, good], np.array([good]), [[0.5], [0.5, 0.5], 0.5]):
        with pytest.raises(ValueError, match=f"runs={R}.*{name}"):
            _call(sa, method, **{name: bad})


@pytest.mark.parametrize("method,name", CASES)
def test_a_bad_element_is_named_by_its_index(sa, method, name):
    good, lo, hi = NUMERIC[method][1][name]
    for what, element in _bad_element(lo, hi):
        for index in (0, R - 1):
            values = list(good)
            values[index] = element
            with pytest.raises(ValueError, match=rf"runs={R}.*{name}\[{index}\]"):
                _call(sa, method, **{name: values})
            if isinstance(element, float):  # the same as an ndarray
                with pytest.raises(ValueError, match=rf"runs={R}.*{name}\[{index}\]"):
                    _call(sa, method, **{name: np.array(values)})


def test_the_ends_of_every_range_are_admitted(intercepted):
    for method, (_, table) in NUMERIC.items():
        for name, (good, lo, hi) in table.items():
            ends = [lo, hi, lo] if lo is not None else [np.nextafter(0.0, 1.0), 1.0e300, 1.0]
            with pytest.raises(Reached):
                _call(intercepted, method, **{name: ends})


def test_strategy_sequences(sa, intercepted):
    from stochopy_amd import _lib

    names = sorted(_lib.DE_STRATEGIES)
    with pytest.raises(KeyError, match="rand3bin"):
        _call(sa, "de", strategy=["rand1bin", "rand3bin", "best1bin"])
    with pytest.raises(KeyError):
        _call(sa, "de", strategy=["rand1bin", 2, "best1bin"])
    for runs in (None, 1):
        with pytest.raises(ValueError, match="(?s)strategy.*runs|runs.*strategy"):
            _call(sa, "de", runs=runs, strategy=names[:R])
    for bad in (names[:2], names, [names[:R]], np.array([names[:R]])):
        with pytest.raises(ValueError, match=f"runs={R}.*strategy"):
            _call(sa, "de", strategy=bad)
    # popsize - 1 >= the largest donor count among the strategies named (rand2bin: 5)
    assert max(_lib.DE_DONORS.values()) == _lib.DE_DONORS["rand2bin"] == 5
    with pytest.raises(ValueError, match=f"runs={R}.*strategy.*rand2bin"):
        _call(sa, "de", popsize=5, strategy=["best1bin", "rand2bin", "rand1bin"])
    with pytest.raises(Reached):
        _call(sa, "de", popsize=6, strategy=["best1bin", "rand2bin", "rand1bin"])
    with pytest.raises(Reached):
        _call(sa, "de", popsize=5, strategy=["best1bin", "best2bin", "rand1bin"])  # four donors at the most


def test_competitivity_none_stays_a_scalar(sa, intercepted):
    with pytest.raises(Reached) as e:
        _call(sa, "cpso", competitivity=None)
    assert e.value.received[10] is None
    with pytest.raises(ValueError, match=rf"runs={R}.*competitivity\[1\]"):
        _call(sa, "cpso", competitivity=[1.0, None, 0.5])


# ---- scalars behave as before


SCALAR_BAD = {
    "de": [("mutation", 2.5), ("mutation", -0.1), ("recombination", 1.5), ("recombination", -0.5)],
    "pso": [("inertia", 1.5), ("cognitivity", 4.5), ("sociability", -1.0)],
    "cpso": [("inertia", -0.5), ("cognitivity", -1.0), ("sociability", 4.5), ("competitivity", 2.5), ("competitivity", -1.0)],
    "cmaes": [("sigma", 0.0), ("sigma", -1.0)],
    "vdcma": [("sigma", 0.0), ("sigma", -1.0)],
}


@pytest.mark.parametrize("method", sorted(SCALAR_BAD))
@pytest.mark.parametrize("runs", [None, R])
def test_a_bad_scalar_raises_the_reference_s_bare_error(sa, method, runs):
    for name, value in SCALAR_BAD[method]:
        for v in (value, np.float64(value), np.array(value)):  # a scalar, a numpy scalar, a 0-d array
            with pytest.raises(ValueError) as e:
                _call(sa, method, runs=runs, **{name: v})
            assert e.value.args == (), (name, v)
    if method == "de":
        with pytest.raises(KeyError) as e:
            _call(sa, method, runs=runs, strategy="rand3bin")
        assert e.value.args == ("rand3bin",)
        with pytest.raises(ValueError) as e:
            _call(sa, method, runs=runs, popsize=3, strategy="rand2bin")
        assert e.value.args == ()


def test_a_bad_scalar_comes_before_a_later_option_s_sequence_error(sa):
    """The order of the reference's checks holds: mutation before recombination before strategy; inertia before
    cognitivity before sociability before competitivity."""
    with pytest.raises(ValueError) as e:
        _call(sa, "de", mutation=3.0, recombination=[0.1, 0.2])  # (the sequence is of the wrong length)
    assert e.value.args == ()
    with pytest.raises(ValueError, match="mutation"):
        _call(sa, "de", mutation=[0.1, 0.2], recombination=3.0, strategy="rand3bin")
    with pytest.raises(ValueError, match="recombination"):
        _call(sa, "de", recombination=[0.1, 0.2], strategy="rand3bin")
    with pytest.raises(ValueError) as e:
        _call(sa, "cpso", inertia=2.0, cognitivity=[0.1, 0.2])
    assert e.value.args == ()
    with pytest.raises(ValueError, match="cognitivity"):
        _call(sa, "cpso", cognitivity=[0.1, 0.2], sociability=5.0, competitivity=[1.0])
    with pytest.raises(ValueError) as e:  # popsize < 2 stands before every hyperparameter
        _call(sa, "de", popsize=1, mutation=[0.1, 0.2])
    assert e.value.args == ()


@pytest.mark.parametrize("method", sorted(NUMERIC))
def test_minimize_runs_receives_arrays_only_for_sequences(intercepted, method):
    """Positions of the hyperparameters in _minimize_runs(R, fun_id, lower, upper, x0, maxiter, P, ...): from 7 on.  A scalar
    arrives as a float (`competitivity`, which may be None, as it was given)."""

    def is_scalar(got, name):
        return np.ndim(got) == 0 if name == "competitivity" else type(got) is float

    table = NUMERIC[method][1]
    names = list(table)
    position = {name: 7 + i for i, name in enumerate(
        {"de": ["mutation", "recombination", "strategy"], "pso": ["inertia", "cognitivity", "sociability", "competitivity"],
         "cpso": ["inertia", "cognitivity", "sociability", "competitivity"], "cmaes": ["sigma"], "vdcma": ["sigma"]}[method])}
    # all scalars (Python floats, numpy scalars and 0-d arrays alike): floats
    scalars = {name: kind(table[name][0][1]) for name, kind in zip(names, [float, np.float64, np.array, np.float32])}
    with pytest.raises(Reached) as e:
        _call(intercepted, method, **scalars)
    for name in names:
        assert is_scalar(e.value.received[position[name]], name), name
    # one sequence at a time, as a list, a tuple and an ndarray; integers are numbers
    for name in names:
        good = table[name][0]
        for given in (list(good), tuple(good), np.array(good), np.array(good, dtype=np.float32)):
            with pytest.raises(Reached) as e:
                _call(intercepted, method, **{name: given})
            got = e.value.received
            for other in names:
                if other == name:
                    assert isinstance(got[position[other]], np.ndarray) and got[position[other]].dtype == np.float64
                    assert np.array_equal(got[position[other]], np.asarray(given, dtype=np.float64))
                else:
                    assert is_scalar(got[position[other]], other), (name, other)
    if method == "de":
        with pytest.raises(Reached) as e:
            _call(intercepted, method, mutation=[0, 1, 2], strategy=("rand1bin", "best2bin", "rand1bin"))
        got = e.value.received
        assert np.array_equal(got[7], [0.0, 1.0, 2.0]) and got[7].dtype == np.float64 and type(got[8]) is float
        assert isinstance(got[9], np.ndarray) and list(got[9]) == ["rand1bin", "best2bin", "rand1bin"]
        with pytest.raises(Reached) as e:
            _call(intercepted, method)
        assert e.value.received[9] == "best1bin"


def test_result_lists_only_what_was_swept():
    from stochopy_amd.optimize import _runs

    out = {"xs": np.array([[1.0, 2.0], [3.0, 4.0]]), "funs": np.array([2.0, 1.0]), "nits": np.array([5, 7]),
           "statuses": np.array([-1, 1], dtype=np.int32)}
    res = _runs.result(dict(out), 4, mutation=0.5, recombination=0.9, strategy="best1bin")
    assert "sweep" not in res and res.run == 1
    F = np.array([0.25, 0.75])
    res = _runs.result(dict(out), 4, mutation=F, recombination=0.9, strategy=np.array(["rand1bin", "best1bin"]))
    assert sorted(res.sweep) == ["mutation", "strategy"]
    assert np.array_equal(res.sweep["mutation"], F) and res.sweep["mutation"] is not F
    assert list(res.sweep["strategy"]) == ["rand1bin", "best1bin"]
    assert res.run == 1 and res.fun == 1.0 and np.array_equal(res.x, [3.0, 4.0]) and res.nfev == 48


# ---- the C ABI


SWEEP_ENTRIES = {
    "sx_de_runs_sweep_launch": "const sx_de_runs_args *a, const double *F, const double *CR, const int32_t *strategy, void *stream",
    "sx_pso_runs_sweep_launch": "const sx_pso_runs_args *a, const double *w, const double *c1, const double *c2, "
                                "const double *gamma, void *stream",
    "sx_cma_runs_sweep_launch": "const sx_cma_runs_args *a, const double *sigma, void *stream",
    "sx_vd_runs_sweep_launch": "const sx_vd_runs_args *a, const double *sigma, void *stream",
}


@pytest.mark.parametrize("name", sorted(SWEEP_ENTRIES))
def test_sweep_entry_points_are_declared_exported_and_bound(lib, name):
    import ctypes as C

    from stochopy_amd import _lib

    header = open(os.path.join(ROOT, "include", "stochopy_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared"
    assert " ".join(m.group(1).split()) == SWEEP_ENTRIES[name]
    assert hasattr(lib, name), f"{name} is not exported"
    restype, argtypes = _lib.PROTOTYPES[name]
    plain, args = _lib.PROTOTYPES[name.replace("_sweep", "")]
    assert restype is C.c_int is plain
    nptr = SWEEP_ENTRIES[name].count(",") - 1  # the per-run arrays between the struct and the stream
    assert argtypes == [args[0]] + [C.c_void_p] * nptr + [args[1]]
    assert getattr(lib, name).argtypes == argtypes


def test_sweep_entry_points_check_their_struct_before_a_device_is_needed(lib):
    """A null struct is refused by the shared code path, whichever entry point it came through."""
    for name in SWEEP_ENTRIES:
        nptr = SWEEP_ENTRIES[name].count(",") - 1
        assert getattr(lib, name)(None, *([None] * nptr), None) != 0
        assert getattr(lib, name.replace("_sweep", ""))(None, None) != 0


def test_existing_structs_did_not_change(lib):
    import ctypes as C

    from stochopy_amd import _lib

    assert [lib.sx_struct_size(i) for i in (8, 9, 10)] == [C.sizeof(_lib.SxDeRunsArgs), C.sizeof(_lib.SxPsoRunsArgs),
                                                           C.sizeof(_lib.SxCmaRunsArgs)]
    assert lib.sx_struct_size(11) == -1 and lib.sx_vd_runs_args_bytes() == C.sizeof(_lib.SxVdRunsArgs)
    assert [C.sizeof(s) for s in (_lib.SxDeRunsArgs, _lib.SxPsoRunsArgs, _lib.SxCmaRunsArgs, _lib.SxVdRunsArgs)] == \
        [152, 192, 232, 256]
