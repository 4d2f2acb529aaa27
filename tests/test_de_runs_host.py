"""DE with options["runs"], host side (no GPU): the C ABI of csrc/sx_de_runs.hip -- struct mirror, the host-only LDS budget --
and the argument checks of optimize.minimize(method="de", options={"runs": R}), all of which raise a ValueError that names
`runs` before a device is needed."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _de_runs_abi  # noqa: E402

LDS_LIMIT = 160 * 1024  # what one workgroup may declare on gfx950


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


def test_struct_mirror_matches_the_library(lib):
    from stochopy_amd import _lib

    assert C.sizeof(_lib.SxDeRunsArgs) == lib.sx_struct_size(8)
    assert _lib.SxDeRunsArgs.R.offset == 9 * 8 and _lib.SxDeRunsArgs.ftol.offset == C.sizeof(_lib.SxDeRunsArgs) - 8


@pytest.mark.parametrize("P,n", [(4, 3), (32, 32), (64, 128)])
def test_lds_budget_of_shapes_that_fit(lib, P, n):
    got = lib.sx_de_runs_lds_bytes(P, n)
    assert 0 < got <= LDS_LIMIT
    assert got >= 2 * P * n * 8  # two generations of the population at the least


def test_lds_budget_refuses_what_does_not_fit(lib):
    assert lib.sx_de_runs_lds_bytes(4096, 128) < 0
    assert lib.sx_de_runs_lds_bytes(1, 8) < 0 and lib.sx_de_runs_lds_bytes(8, 0) < 0  # not a population / not a row
    assert lib.sx_de_runs_lds_bytes(4, lib.sx_wide_from() + 1) < 0                     # rows the wide kernels serve


R, P, N = 3, 8, 5
BASE = {"runs": R, "popsize": P, "maxiter": 4, "seed": 0, "rng": "philox", "updating": "deferred"}


def _call(sa, fun=None, x0=None, callback=None, n=N, **changes):
    opts = dict(BASE, **changes)
    return sa.optimize.minimize(fun if fun is not None else sa.factory.sphere, [[-5.12, 5.12]] * n, x0=x0, method="de",
                                options=opts, callback=callback)


BAD = {
    "numpy-legacy rng": lambda sa: _call(sa, rng="numpy-legacy"),
    "default rng": lambda sa: _call(sa, rng=None),
    "batched objective": lambda sa: _call(sa, fun=sa.factory.batched(lambda X: (X * X).sum(dim=1))),
    "plain lambda": lambda sa: _call(sa, fun=lambda x: float(np.sum(x * x))),
    "workers=2": lambda sa: _call(sa, workers=2),
    "callback": lambda sa: _call(sa, callback=lambda X, res: None),
    "return_all": lambda sa: _call(sa, return_all=True),
    "runs=0": lambda sa: _call(sa, runs=0),
    "runs=-2": lambda sa: _call(sa, runs=-2),
    "runs=2.5": lambda sa: _call(sa, runs=2.5),
    "seed sequence of the wrong length": lambda sa: _call(sa, seed=[1, 2]),
    "no seed": lambda sa: _call(sa, seed=None),
    "x0 (R+1, P, n)": lambda sa: _call(sa, x0=np.zeros((R + 1, P, N))),
    "P x n beyond the LDS": lambda sa: _call(sa, popsize=4096, n=128),
    "rows beyond the narrow kernels": lambda sa: _call(sa, n=2049),
    "strict immediate": lambda sa: _call(sa, updating="immediate", strict_updating=True),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_argument_checks_name_runs_and_need_no_device(sa, what):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (a plain callable's host-evaluation note is not what is tested)
        with pytest.raises(ValueError, match="runs"):
            BAD[what](sa)


def test_immediate_updating_defers_with_a_warning_unless_told_otherwise(sa):
    """updating="immediate" cannot be an ordered sweep of R runs: strict_updating=None says so in a warning, False is
    silent; either way the call then goes on -- here into the next check, which needs no device either."""
    with pytest.warns(RuntimeWarning, match="deferred"):
        with pytest.raises(ValueError, match="runs"):
            _call(sa, updating="immediate", return_all=False, seed=[1])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="runs"):
            _call(sa, updating="immediate", strict_updating=False, seed=[1])


def test_reference_checks_still_come_first(sa):
    """The reference's own argument checks (de/_de.py:116-140) are not displaced by the new option."""
    with pytest.raises(ValueError):
        _call(sa, mutation=3.0)
    with pytest.raises(KeyError):
        _call(sa, strategy="rand3bin")
    with pytest.raises(ValueError):
        _call(sa, popsize=3, strategy="rand2bin")  # five donors out of two other rows
    with pytest.raises(ValueError):
        _call(sa, x0=np.zeros((P + 1, N)))


@pytest.mark.parametrize("n", [3, 64, 256, 257, 1024, 2048])
def test_lds_budget_at_its_limit(lib, sa, n):
    """The largest population sx_de_runs_lds_bytes accepts for rows of n elements: within 160 KiB, one row more refused,
    strictly increasing below it, and everywhere the bytes of the layout the kernel's header comment documents --
    buf[2][P][stride] | fit[P] | 4 broadcast words, stride = n + 8 up to 256 elements, n + 8 + 2 (n // 64 + 2) above (the
    broadcast words are the LAST bytes of the run's LDS: a budget short of them is a write past it).  The front end refuses
    the first population that does not fit, before a device is needed."""
    pmax = _de_runs_abi.largest_popsize(lib, n)
    stride = n + 8 if n <= 256 else n + 8 + 2 * (n // 64 + 2)
    assert _de_runs_abi.stride_doubles(n) == stride
    top = lib.sx_de_runs_lds_bytes(pmax, n)
    assert 0 < top <= 163840 == LDS_LIMIT
    assert lib.sx_de_runs_lds_bytes(pmax + 1, n) < 0
    assert 8 * (2 * (pmax + 1) * stride + (pmax + 1) + 4) > LDS_LIMIT  # pmax + 1 is refused because it does not fit
    got = np.array([lib.sx_de_runs_lds_bytes(P, n) for P in range(2, pmax + 1)], dtype=np.int64)
    assert (np.diff(got) > 0).all()
    P = np.arange(2, pmax + 1, dtype=np.int64)
    assert np.array_equal(got, 8 * (2 * P * stride + P + 4))
    with pytest.raises(ValueError, match="runs.*LDS.*160 KiB"):  # the budget check, not an earlier refusal
        _call(sa, runs=2, popsize=pmax + 1, n=n, strategy="rand1bin")
