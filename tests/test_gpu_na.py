"""GPU parity: the Neighbourhood Algorithm (csrc/sx_na.hip: the cell walks on the device; ranking and the scalar d1
recurrence on the host) against vectors captured from the reference (numpy-legacy draws) and against the oracle
(Philox draws).  Mirrors the reference's own NA test row (tests/test_optimize.py:89-92)."""
import os

import numpy as np
import pytest

import oracle
from conftest import GOLDEN, case_bounds, load_golden, unhex

pytestmark = pytest.mark.gpu

EXACT = {"rosenbrock", "sphere"}  # + - * only: the objective's bits are numpy's
CASES = load_golden("na.json")["cases"]
EDGE_CASES = load_golden("na_edges.json")["cases"]


@pytest.fixture(scope="module")
def sa():
    import stochopy_amd

    return stochopy_amd


def _matches_reference_golden(sa, case, npz):
    trace = []
    opts = dict(case["options"], backend="hip", rng="numpy-legacy")
    res = sa.optimize.minimize(getattr(sa.factory, case["objective"]), case_bounds(case), x0=case["x0"], method="na",
                               options=opts, callback=lambda X, r: trace.append(float(r.fun)))
    ref = case["result"]
    arrays = np.load(os.path.join(GOLDEN, npz))
    assert (res.nit, res.nfev, res.status, res.success, res.message) == (
        ref["nit"], ref["nfev"], ref["status"], ref["success"], ref["message"])
    if case["objective"] in EXACT:
        assert np.array_equal(res.x, unhex(ref["x"])) and res.fun == unhex(ref["fun"])
        assert np.array_equal(np.array(trace), unhex(case["fun_trace"]))
        assert np.array_equal(res.xall, arrays[case["tag"] + "__xall"])
        assert np.array_equal(res.funall, arrays[case["tag"] + "__funall"])
    else:
        assert np.allclose(res.x, unhex(ref["x"]), rtol=1e-9, atol=1e-12) and np.isclose(res.fun, unhex(ref["fun"]), rtol=1e-9)
        assert np.allclose(trace, unhex(case["fun_trace"]), rtol=1e-9)
        assert np.allclose(res.xall, arrays[case["tag"] + "__xall"], rtol=1e-9, atol=1e-12)
    if "xref_from_reference_tests" in case:
        assert np.allclose(case["xref_from_reference_tests"], res.x)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["tag"])
def test_na_matches_reference_golden(sa, case):
    """numpy-legacy stream: same seed => the reference's run.  For + - * objectives everything is bit-identical
    (result, per-generation best-f, the history incl. the normalised rows the reference stores at iteration 1); with
    cos / exp in the objective the fitness VALUES differ from libm's by ulps, the samples only if a ranking flips."""
    _matches_reference_golden(sa, case, "na_xall.npz")


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: c["tag"])
def test_na_matches_reference_golden_at_the_walk_edges(sa, case):
    """The same on runs whose cell walks are degenerate (tests/golden/na_edges.*; all + - * objectives, so bit for bit):
    a fixed axis first, last, next to another one; duplicate rows and a constant column in x0, or all rows equal (NaN
    and infinite walls, axes without any wall); 70 samples a generation (the draw kernel's second workgroup); one axis."""
    assert case["objective"] in EXACT
    _matches_reference_golden(sa, case, "na_edges_xall.npz")


@pytest.mark.parametrize("cfg", [("rosenbrock", 2, 8, 60, 0.5), ("sphere", 6, 24, 25, 0.25), ("rosenbrock", 17, 40, 12, 1.0),
                                 ("sphere", 140, 12, 6, 0.5)], ids=lambda c: "%s_n%d_p%d" % c[:3])
def test_na_philox_vs_oracle(sa, cfg):
    """In-kernel-style draws (Philox keyed by sample / generation / axis): bit-identical to the oracle, incl. rows of more
    than 128 axes (the pairwise order of the initial cell distances recurses)."""
    obj, n, P, maxiter, nrperc = cfg
    bounds = [[-3.0, 4.0]] * n
    opts = {"maxiter": maxiter, "popsize": P, "seed": 99 + n, "nrperc": nrperc, "return_all": True}
    ref = oracle.minimize(obj, bounds, method="na", options=dict(opts), rng="philox")
    got = sa.optimize.minimize(getattr(sa.factory, obj), bounds, method="na", options=dict(opts, backend="hip", rng="philox"))
    assert (got.nit, got.status) == (ref.nit, ref.status) and got.fun == ref.fun and np.array_equal(got.x, ref.x)
    assert np.array_equal(got.xall, ref.xall) and np.array_equal(got.funall, ref.funall)


def _philox_vs_oracle(sa, obj, bounds, opts, x0=None):
    opts = dict(opts, return_all=True)
    ref = oracle.minimize(obj, bounds, x0=x0, method="na", options=dict(opts), rng="philox")
    got = sa.optimize.minimize(getattr(sa.factory, obj), bounds, x0=x0, method="na",
                               options=dict(opts, backend="hip", rng="philox"))
    assert (got.nit, got.status) == (ref.nit, ref.status) and got.fun == ref.fun and np.array_equal(got.x, ref.x)
    assert np.array_equal(got.xall, ref.xall) and np.array_equal(got.funall, ref.funall)
    return got


@pytest.mark.parametrize("cfg", [("rosenbrock", 3, 70, 12, 0.3), ("sphere", 2, 130, 8, 1.0), ("sphere", 1, 12, 10, 0.5),
                                 ("rosenbrock", 258, 6, 4, 0.5)], ids=lambda c: "%s_n%d_p%d" % c[:3])
def test_na_philox_vs_oracle_at_the_walk_edges(sa, cfg):
    """More samples than one workgroup of the draw kernel serves (70: two; 130: three, every model a cell centre), a
    single axis (no term in the cell distances, no recurrence), and 257 terms (the pairwise sum splits, and its right half
    is again longer than a leaf)."""
    obj, n, P, maxiter, nrperc = cfg
    _philox_vs_oracle(sa, obj, [[-3.0, 4.0]] * n, {"maxiter": maxiter, "popsize": P, "seed": 99 + n, "nrperc": nrperc})


FIXED_BOUNDS = [[[1.5, 1.5], [-2, 3], [-1, 1], [-5, 5]], [[-2, 3], [-1, 1], [-5, 5], [.5, .5]],
                [[-2, 3], [1, 1], [2, 2], [-5, 5]], [[1, 1], [2, 2], [-1, 2]]]


@pytest.mark.parametrize("k", range(len(FIXED_BOUNDS)), ids=["first", "last", "adjacent", "leading_pair"])
def test_na_philox_fixed_axes_vs_oracle(sa, k):
    """A fixed axis first, last, next to another one, and two in front: the store holds the bound there in the first
    generation and 0.0 afterwards, and the deferred update of the cell distances reads axis jp + 1 whether free or not."""
    bounds = [[float(a), float(b)] for a, b in FIXED_BOUNDS[k]]
    _philox_vs_oracle(sa, ("sphere", "rosenbrock")[k % 2], bounds, {"maxiter": 15, "popsize": 12, "seed": 61 + k, "nrperc": 0.5})


def _degenerate_x0(which):
    if which == "duplicates_flat_column":  # rows 5 and 7 equal to row 2, column 1 constant
        x0 = np.random.RandomState(71).uniform(-3.0, 4.0, (12, 3))
        x0[:, 1] = 0.75
        x0[5] = x0[7] = x0[2]
        return x0
    return np.tile(np.random.RandomState(72).uniform(-3.0, 4.0, 3), (12, 1))


@pytest.mark.parametrize("which", ["duplicates_flat_column", "all_equal"])
def test_na_philox_degenerate_x0_vs_oracle(sa, which):
    """Copies of a cell centre among the models (0 / 0: a NaN wall that neither comparison may take) and an axis on
    which every model has the centre's coordinate (infinite walls); with all rows equal the first walks meet no wall."""
    _philox_vs_oracle(sa, ("rosenbrock", "sphere")[which == "all_equal"], [[-3.0, 4.0]] * 3,
                      {"maxiter": 15, "popsize": 12, "seed": 73, "nrperc": 0.5}, x0=_degenerate_x0(which))


def test_na_with_a_plain_python_objective_and_validation(sa):
    """Any callable works (evaluated per individual on the host); the reference's validation rules hold."""
    import warnings

    f = lambda x: float(np.sum((x - 0.5) ** 2))  # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        res = sa.optimize.minimize(f, [[-2.0, 2.0]] * 3, method="na", options={"maxiter": 40, "popsize": 16, "seed": 1})
    assert res.fun < 1e-2 and np.allclose(res.x, 0.5, atol=0.1)
    b = [[-1.0, 1.0]] * 2
    for bad in ({"popsize": 1}, {"nrperc": 0.0}, {"nrperc": 1.5}):
        with pytest.raises(ValueError):
            sa.optimize.minimize(sa.factory.sphere, b, method="na", options=bad)
    with pytest.raises(ValueError):
        sa.optimize.minimize(sa.factory.sphere, b, x0=np.zeros((3, 2)), method="na", options={"popsize": 8})
