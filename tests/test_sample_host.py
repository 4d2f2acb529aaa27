"""Samplers, host side (no GPU): the numpy restatement (tests/_sample_oracle.py) reproduces the reference's recorded runs
(tests/golden/sample.json / sample_xall.npz) bit for bit in numpy-legacy mode, and stochopy_amd.sample's argument checks
raise before a device is needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _sample_oracle  # noqa: E402
from conftest import GOLDEN, load_golden, unhex  # noqa: E402

CASES = load_golden("sample.json")["cases"]


def case_setup(case):
    bounds = [case["bounds"]] * case["ndim"]
    x0 = None if case["x0"] is None else unhex(case["x0"])
    return bounds, x0


def check_callback_records(records, want, exact, span=10.24):
    """The per-call state of a run against the reference's: counts exact, floats bit for bit (`exact`) or within the
    parity tolerances (1e-6 of the search range / 1e-6 relative)."""
    assert len(records) == len(want)
    for got, ref in zip(records, want):
        assert (got["nit"], got["len_xall"], got["len_funall"]) == (ref["nit"], ref["len_xall"], ref["len_funall"])
        assert got["accept_ratio"] == unhex(ref["accept_ratio"])
        for key, scale in (("xk", span), ("x", span), ("fun", None)):
            a, b = np.asarray(got[key]), unhex(ref[key])
            if exact:
                assert np.array_equal(a, b), (ref["nit"], key)
            elif scale is None:
                assert np.allclose(a, b, rtol=1e-6, atol=0), (ref["nit"], key)
            else:
                assert np.allclose(a, b, rtol=0, atol=1e-6 * scale), (ref["nit"], key)


def recorder(records):
    def cb(xk, state):
        records.append({"nit": int(state.nit), "fun": float(state.fun), "accept_ratio": float(state.accept_ratio),
                        "x": np.array(state.x, copy=True), "xk": np.array(xk, copy=True),
                        "len_xall": len(state.xall), "len_funall": len(state.funall)})

    return cb


@pytest.mark.parametrize("case", CASES, ids=[c["tag"] for c in CASES])
def test_restatement_reproduces_the_reference(case):
    arrays = np.load(os.path.join(GOLDEN, "sample_xall.npz"))
    bounds, x0 = case_setup(case)
    records = []
    saved = np.random.get_state()
    try:
        with np.errstate(all="ignore"):
            res = _sample_oracle.sample(case["objective"], bounds, x0=x0, method=case["method"],
                                        options=dict(case["options"], rng="numpy-legacy"),
                                        callback=recorder(records) if "callback" in case else None)
        after = np.random.rand(4)
    finally:
        np.random.set_state(saved)
    ref = case["result"]
    assert np.array_equal(res.xall, arrays[case["tag"] + "__xall"])
    assert np.array_equal(res.funall, arrays[case["tag"] + "__funall"])
    assert np.array_equal(res.x, unhex(ref["x"])) and float(res.fun) == unhex(ref["fun"])
    assert res.nit == ref["nit"] and res.accept_ratio == unhex(ref["accept_ratio"])
    if case["method"] == "hmc":
        assert res.nfev == ref["nfev"]
    assert np.array_equal(after, unhex(case["next_draws"]))  # numpy's global stream is where the reference leaves it
    if "callback" in case:
        check_callback_records(records, case["callback"], exact=True)


def test_restatement_gradients_match_finite_differences():
    """The closed forms the GPU tests compare the kernel's gradients with, against central differences of the oracle's
    objectives (truncation error O(h^2) with h = 1e-5, rounding ~1e-16 f / h: 1e-5 of the gradient's norm covers both)."""
    from oracle import objectives

    rs = np.random.RandomState(5)
    for name, grad in _sample_oracle.GRADIENTS.items():
        X = rs.uniform(-3.0, 3.0, (4, 7))
        g = grad(X)
        f = objectives.OBJECTIVES[name]
        h = 1e-5
        num = np.empty_like(X)
        for i in range(X.shape[1]):
            Xp, Xm = X.copy(), X.copy()
            Xp[:, i] += h
            Xm[:, i] -= h
            num[:, i] = (f(Xp) - f(Xm)) / (2 * h)
        assert np.all(np.linalg.norm(g - num, axis=1) <= 1e-5 * np.linalg.norm(g, axis=1)), name


def test_philox_restatement_does_not_depend_on_the_number_of_chains():
    opts = {"maxiter": 30, "seed": 9, "rng": "philox", "stepsize": 0.05}
    b = [[-5.12, 5.12]] * 6
    few = _sample_oracle.sample("rastrigin", b, method="mcmc", options=dict(opts, chains=3))
    many = _sample_oracle.sample("rastrigin", b, method="mcmc", options=dict(opts, chains=9))
    assert np.array_equal(few.xall[2], many.xall[2]) and np.array_equal(few.funall[2], many.funall[2])


def test_argument_checks_need_no_device():
    import stochopy_amd as sa

    sphere, b = sa.factory.sphere, [[-1.0, 1.0]] * 4

    def raises(exc, method="mcmc", fun=sphere, bounds=b, x0=None, args=(), **options):
        with pytest.raises(exc):
            sa.sample.sample(fun, bounds, x0=x0, args=args, method=method, options=options)

    # what the reference raises
    for method in ("mcmc", "hmc"):
        raises(TypeError, method, fun=1.0)
        raises(ValueError, method, bounds=[-1.0, 1.0])
        raises(ValueError, method, x0=[0.0, 0.0, 0.0])
        raises(ValueError, method, stepsize=[0.1, 0.1])
    raises(ValueError, "mcmc", perc=1.5)
    raises(ValueError, "mcmc", perc=-0.1)
    raises(ValueError, "hmc", nleap=0)
    with pytest.raises(ValueError):
        sa.sample.sample(sphere, b, callback=3)
    # this backend's own
    for method in ("mcmc", "hmc"):
        with pytest.raises(TypeError, match="factory"):
            sa.sample.sample(lambda x: float(np.sum(x * x)), b, method=method)
        raises(TypeError, method, fun=sa.factory.batched(lambda X: X.sum(1)))
        raises(ValueError, method, bounds=[[-1.0, 1.0]] * 2049)
        raises(ValueError, method, chains=2)  # numpy-legacy is the default
        raises(ValueError, method, chains=0, rng="philox", seed=1)
        raises(ValueError, method, constraints="Reject")
        raises(ValueError, method, rng="philox")  # no seed
        raises(ValueError, method, rng="mt")
        raises(ValueError, method, backend="cpu")
        raises(ValueError, method, x0=np.zeros((3, 4)), chains=2, rng="philox", seed=1)
    raises(TypeError, "hmc", jac=lambda x: 2.0 * x)
    raises(TypeError, "hmc", jac="numeric")


def test_sample_is_part_of_the_package():
    import stochopy_amd as sa
    from stochopy_amd import _lib

    assert sa.sample.sample is sa.sample._helpers.sample and issubclass(sa.sample.SampleResult, dict)
    assert set(sa.sample._helpers._sampler_map) == {"mcmc", "hmc"}
    import ctypes

    assert ctypes.sizeof(_lib.SxSampleArgs) == _lib.lib().sx_struct_size(7)
    # launch geometry: several chains per workgroup, within the 16-row cap of the row kernels
    for method, jac in ((0, 0), (1, 0), (1, 1)):
        for n in (3, 64, 128, 256, 2048):
            assert 1 <= _lib.lib().sx_sample_chains_per_workgroup(method, jac, n) <= 16
    assert _lib.lib().sx_sample_chains_per_workgroup(0, 0, 128) == 16
